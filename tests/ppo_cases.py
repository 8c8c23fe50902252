"""Test helper: seeded cases for the fused PPO minibatch gradient (pime_ppo_minibatch_grad / _step: csrc/ppo_fused.hip,
csrc/mlp16.hip, csrc/ppo_train.hip), their kink margins and oracle mutants, in the mould of tests/td3_cases.py and
tests/sac_cases.py.  Shared by tests/test_ppo_cases_cpu.py and tests/test_gpu_ppo_sweep.py so that the CPU tests see bit for bit
what the GPU tests run.

The same numbers as in the two other case modules rule the inputs (conditions on the INPUTS, checked on the CPU; none is a
tolerance on a kernel):

  * DELTA = 1e-5, the kink margin.  The objective is not differentiable where ratio = 1 + clip under a positive advantage or
    1 - clip under a negative one (the side on which the clip is live), where |v - r_sum| = 1 and where a ReLU pre-activation of
    the critic is 0.  Table rows whose relative distance to such a point is below DELTA are redrawn; at most MAX_REDRAWN of a case's
    table may be (a cap, not a measurement).
  * MUTATION_MARGIN = 10 (x the 3e-4 bar): every mutant of ppo_oracle.MUTANTS must move at least one gradient tensor of every
    vetted case of 32 samples or more by 10 x the bar.  Two conditions on the inputs make that possible.  The entropy proxy
    enters the gradient with weight lambda_entropy next to advantages of order 1; at the agent's 0.02 it moves the gradients by
    well under 1 % -- below 10 x the bar on most tensors -- so the cases run at LAMBDA_ENTROPY = 0.5 (an argument of the call,
    like the clip of 0.2).  And the branches have to be populated, which the reference's own initialisation and a random table do
    not do (tests/test_gpu_ppo_fused.py: r_sum ~ N(-40, 30) against a critic near 0 leaves 97 % of the samples in the linear
    SmoothL1 branch): see the generator below.
  * F32_STABILITY = 1e-4: the oracle in float32 numpy must agree with float64 to that much of each gradient tensor's largest
    entry.

The generator.  Nets are seeded, not the reference's initialisation: every hidden layer is rescaled so that its pre-activations
have standard deviation 1 on probe rows (Tanh units well into their curved part, about half of the ReLU units closed), the actor's
head to a mean of standard deviation 1, the critic's head to a value of standard deviation 1; a_std_log = -0.3.  The trajectory
table has N_ROWS = 2 048 rows; row i belongs to combination i mod 10 of

    ratio category   unclipped (ratio in [0.85, 1.15]) | above 1 + clip with adv > 0 (clip live) | above with adv < 0 |
                     below 1 - clip with adv < 0 (clip live) | below with adv > 0
  x SmoothL1 branch  quadratic (|v - r_sum| in [0.1, 0.9]) | linear (in [1.1, 3])

and is made to sit there: the stored old log-prob is the policy's own log-prob of the stored action shifted by -log of a ratio
drawn inside the category, r_sum is v(s) plus an offset drawn inside the branch.  Position p of the index list draws a row of
combination p mod 10, so every case of 32 samples or more holds at least 10 % of its samples in each ratio category and 20 % in
each SmoothL1 branch whatever the seed (tests/test_ppo_cases_cpu.py asserts it).  Positions 0 and B - 1 name row 0 and the last
row, position 11 repeats position 1's row (position 2 does below 13 samples), and random repeats occur besides.

The last row of the table, which position B - 1 names, carries an advantage of max(1, 10 sqrt(B) / 256): one sample's share of
a sum of B terms of either sign falls as 1 / sqrt(B), so a kernel that lost the last sample of a 65 537-sample batch would stay
under the bar on ordinary data; at 10 typical advantages it does not (the mutant "drop_last_sample").  Up to 655 samples the row
is an ordinary one.

B = 1 is left out of every list: the reference's scale 1 / (r_sum.std() + 1e-5) is NaN for one sample (unbiased std), so there
is nothing for the oracle to be compared with.  The smallest batch is 2.

Routes.  A spec names the route it expects -- (actor's family, critic's family, launch form) -- from the model `expected_route`
below, which is written down from csrc (fused_lds / pair_lds against 160 KB) and held against pime_ppo_route for every swept
shape by the CPU test.  What the model says, and what was not obvious from reading the kernels: at width 128 the pair kernel
serves D = 1..4 and D = 8, the dual kernel D = 5..7 and 9..13 (the 8-float padded rows of first_grad_valu take the LDS that the
merged map lacks; D = 8 has no padded rows), the 16-tile family (plain nets) or the split pipeline (modular actor) D >= 14; at
width 64 the pair kernel serves every D <= 32; width 256 is always the 16-tile family."""
import collections
import functools
import os
import re

import numpy as np

import ppo_oracle as P

DELTA = 1e-5
BAR = 3e-4
MUTATION_MARGIN = 10.0
F32_STABILITY = 1e-4
MAX_REDRAWN = 0.10

RATIO_CLIP = 0.2
LAMBDA_ENTROPY = 0.5
A_STD_LOG = -0.3
N_ROWS = 2048
WIDTHS = (64, 128, 256)
MAX_D = 32

RATIO_CATEGORIES = ("unclipped", "above_live", "above_dead", "below_live", "below_dead")
L1_BRANCHES = ("quadratic", "linear")

Spec = collections.namedtuple("Spec", "kind D Di aw cw B route vet")
# kind: "plain" (ActorResidualPPO) | "ppo" (ActorPPO: the same net under another class) | "modular"


# ------------------------------------------------------------------------------------------------------------------ routes
def net_family(kind, width, D, forced16=False):
    """The family that serves one net: "16tile" | "lds" | "split".  kind: "critic" | "plain" | "modular"."""
    if width == 256:
        return "16tile"
    if forced16 and (kind != "modular" or width == 128):   # PIME_MLP16=1: every plain net, and the modular actor at width 128
        return "16tile"
    if width == 64 or D <= 13:
        return "lds"
    return "split" if kind == "modular" else "16tile"


# PIME_GRAD_BF16X3=1 (read once per process, like PIME_MLP16): the nets of the 16-tile family at widths 128 / 256 run the
# B3 = true kernels (b3_grad of csrc/mlp16.hip = the variable && width 128 / 256 && family16_grad).  One shape then has no kernel
# at all (ppo16_fits): ppo16m_kernel<16, true> asks for lds16m<16>(D, Di, true, true).total floats of LDS --
#   the region, max over the streamed layers' slice buffers and the dW rounds: Dw16SlicedB3<16>::FLOATS =
#     3 planes x 64 rows x (16 + 4 tiles) x 32 B = 122 880 B (the f32 kernel's own region is smaller, which is why it fits);
#   the two first-layer images, 16 tiles x 64 lanes x 4 floats = 4 096 B per k-step of 4 inputs: ceil((D - Di) / 4) + ceil(Di / 4);
#   biases, head and the waves' sums: 256 + 128 + 256 + 128 + 256 + 256 + 4 + 48 floats = 5 328 B
# -- against 160 KB = 163 840 B: 35 632 B are left for the first layer, 8 k-steps.  Di <= 3 takes one, so the plant tower has 7:
# D - Di <= 28 is served, a tower of 29 floats or more is not.
B3_MAX_TOWER_256 = (163840 - 122880 - 5328) // 4096 * 4 - 4
assert B3_MAX_TOWER_256 == 28


def b3_process():
    """Does this process run the variant?  (The library's own reading of the variable: set, and atoi of it not 0.)"""
    m = re.match(r"\s*[+-]?\d+", os.environ.get("PIME_GRAD_BF16X3", ""))
    return bool(m) and int(m.group()) != 0


def forced16_process():
    return os.environ.get("PIME_MLP16") is not None


def b3_net(kind, width, D, Di=0, forced16=False):
    """Under PIME_GRAD_BF16X3=1: does this net run a B3 = true kernel (and carry bf16 planes behind its transposed image)?  Every net
    of width 256; at width 128 the nets of the 16-tile family -- plain actors and critics on 14 floats or more, and under PIME_MLP16=1
    everything, the modular actor included; never at width 64, never a net of the LDS-resident or the split family.  (True as well
    for the one shape the variant does not serve: its image is sized before the launch refuses.)"""
    return width in (128, 256) and net_family(kind, width, D, forced16) == "16tile"


def expected_route(kind, D, Di, aw, cw, forced16=False, b3=False):
    """(actor's family, critic's family, launch form "pair" | "dual" | "single").  b3: under PIME_GRAD_BF16X3=1, where the actor's
    family is "none" for a modular actor of width 256 with a plant tower above B3_MAX_TOWER_256 (pime_ppo_route refuses it)."""
    fa = net_family("modular" if kind == "modular" else "plain", aw, D, forced16)
    fc = net_family("critic", cw, D, forced16)
    if b3 and kind == "modular" and aw == 256 and D - Di > B3_MAX_TOWER_256:
        fa = "none"
    launch = "single"
    if fa == fc == "lds" and aw == cw:
        launch = "pair" if (aw == 64 or D <= 4 or D == 8) else "dual"
    return fa, fc, launch


def library_route(kind, D, Di, aw, cw):
    """The same triple from the library (pime_ppo_route: host-only, the function pime_ppo_minibatch_grad dispatches on; it follows
    the process's PIME_MLP16)."""
    import ctypes
    import pime_amd.native as nt
    r = (ctypes.c_int32 * 3)()
    k = nt.MLP_MODULAR_ACTOR if kind == "modular" else nt.MLP_PLAIN_ACTOR
    rc = nt.lib().pime_ppo_route(k, D, Di if kind == "modular" else 0, aw, cw, r)
    families = ("16tile", "lds", "split", "none")
    if rc != 0 and "none" not in (families[r[0]], families[r[1]]):   # a net without a kernel is an answer (the query fills the
        nt.check(rc, "pime_ppo_route")                                 # triple, then refuses); anything else is an error
    assert (rc != 0) == ("none" in (families[r[0]], families[r[1]]))
    return families[r[0]], families[r[1]], ("single", "dual", "pair")[r[2]]


def first_layer_class(family, kind, D):
    """The first-layer variant a net takes inside its family: the LDS-resident kernels pad the state rows to 4 / 8 floats for
    first_grad_valu or use the matrix form (first_valu_pad); the plain 16-tile kernels lay the first layer out in one or two
    blocks of 16 columns (tb0 of slab_layout16); the modular 16-tile kernel and the split pipeline have one form."""
    if family == "lds":
        return "pad4" if D <= 3 else "pad8" if D <= 7 else "matrix"
    if family == "16tile" and kind != "modular":
        return "tb1" if D <= 16 else "tb2"
    return "one"


def kernel_class(s, forced16=False):
    """(route, actor width, critic width, actor kind, first-layer class of the actor, of the critic)."""
    k = "modular" if s.kind == "modular" else "plain"
    route = expected_route(s.kind, s.D, s.Di, s.aw, s.cw, forced16)
    return route, s.aw, s.cw, k, first_layer_class(route[0], k, s.D), first_layer_class(route[1], "critic", s.D)


def spec(kind, D, Di, aw, B, cw=None, vet=True):
    cw = aw if cw is None else cw
    return Spec(kind, D, Di if kind == "modular" else 0, aw, cw, B, expected_route(kind, D, Di, aw, cw), vet)


def spec_id(s):
    tag = f"{s.kind}-{s.aw}" + (f"+{s.cw}" if s.cw != s.aw else "") + f"-D{s.D}" + (f"i{s.Di}" if s.kind == "modular" else "")
    return f"{tag}-B{'cap' if s.B == CAP_B else s.B}-{s.route[2]}" + ("" if s.vet else "-unvetted")


CAP_B = 0   # placeholder of the variant's lists: "grid x 64 + 1", resolved where the grid can be read (resolve_cap)


def shape_cases():
    """Widths 64 / 128 / 256 x {plain D 1..32, modular D 2..32 with Di 1} at B = 37 (a full 32-tile and a ragged one; two 16-tiles
    and a ragged one), modular Di 2 and 3 once per width, ActorPPO once."""
    out = []
    for w in WIDTHS:
        out += [spec("plain", D, 0, w, 37) for D in range(1, MAX_D + 1)]
        out += [spec("modular", D, 1, w, 37) for D in range(2, MAX_D + 1)]
        out += [spec("modular", D, Di, w, 37) for D, Di in ((4, 2), (7, 3))]
    out.append(spec("ppo", 3, 0, 128, 37))
    return out


FUSED_CAP = 256   # workgroups of the LDS-resident kernels (pime_ppo_fused_grid); the GPU test reads it from the library
GRID16_CAP = 256  # ... of the 16-tile kernels at the swept shapes (pime_ppo_grid16)
# fewer than one tile | a tile - 1 | a tile + 1 | a group - 1 | a group + 1 (LDS-resident: 32-sample tiles, 8 per workgroup -- at 33 and
# 257 the last workgroup runs one valid tile and seven clamped ones; 16-tile: 16-sample tiles, 64-sample groups; split: 32-sample tiles)
REGIME_B = {"lds": (2, 31, 33, 255, 257), "16tile": (2, 15, 17, 63, 65), "split": (2, 31, 33, 255, 257)}


def _class_representatives(cases, forced16=False):
    seen = {}
    for s in cases:
        seen.setdefault(kernel_class(s, forced16), s)
    return seen


def regime_cases():
    """Every kernel class of the shape list (its first member) at every batch size of REGIME_B for the families it runs on, and one
    batch of grid cap x group + 1 (a workgroup takes a second group and accumulates into its slab) per (route, widths)."""
    out, capped = [], set()
    for cls, s in _class_representatives(shape_cases()).items():
        route = cls[0]
        for B in sorted({b for fam in route[:2] for b in REGIME_B[fam]}):
            out.append(s._replace(B=B))
        if (route, s.aw) not in capped:
            capped.add((route, s.aw))
            big = max(FUSED_CAP * 256 + 1 if "lds" in route[:2] else 0, GRID16_CAP * 64 + 1 if "16tile" in route[:2] else 0,
                      GRID16_CAP * 64 + 1 if "split" in route[:2] else 0)
            out.append(s._replace(B=big))
    return out


def mixed_cases():
    """Actor and critic of different widths: every net in a launch of its own (ppo_fused_kernel<T, KIND> by itself)."""
    out = []
    for B in (37, 257):
        out += [spec("plain", 3, 0, 64, B, cw=128), spec("modular", 5, 2, 128, B, cw=64), spec("plain", 9, 0, 256, B, cw=128)]
    return out


def forced16_cases():
    """Run in a child process under PIME_MLP16=1 (read once per process): widths 64 / 128 through the 16-tile family."""
    out = []
    for B in (37, 65):
        for w in (64, 128):
            out += [spec("plain", 3, 0, w, B), spec("plain", 20, 0, w, B), spec("modular", 4, 1, w, B)]
        out.append(spec("modular", 20, 1, 128, B))   # a plant tower of 19 floats: two first-layer column tiles in ppo16m_kernel<8>
    return [s._replace(route=expected_route(s.kind, s.D, s.Di, s.aw, s.cw, forced16=True)) for s in out]


def per_route_shapes():
    """One shape per (route, widths): the first of the shape list and of the mixed list."""
    seen = {}
    for s in shape_cases() + mixed_cases():
        seen.setdefault((s.route, s.aw, s.cw), s)
    return list(seen.values())


def property_cases():
    """The batches of the bit-level properties (poisoned rows, stale slabs, frozen parameters), which are also held to the oracle:
    293 = a second workgroup of the LDS-resident kernels with one full tile, a ragged one and six clamped ones, a ragged 16-tile;
    100 = what follows a launch at 4 096 on the same object."""
    return [s._replace(B=B) for s in per_route_shapes() for B in (293, 100)]


def gradient_specs():
    seen = []
    for s in shape_cases() + regime_cases() + mixed_cases() + property_cases():
        if s not in seen:
            seen.append(s)
    return seen


# ------------------------------------------------------------------------------------------- the bf16x3 variant's lists
# Run in child processes under PIME_GRAD_BF16X3=1 (tests/test_gpu_ppo_sweep.py part f, tests/test_gpu_ppo_chain.py).  A spec's
# route is the variant's (expected_route(..., b3=True)); where a shape, batch and route are those of an f32 list the spec IS that
# list's spec, and the case -- seeded from the shape and the batch alone -- is the same one.
def b3_spec(kind, D, Di, aw, B, cw=None, forced16=False, vet=True):
    s = spec(kind, D, Di, aw, B, cw, vet)
    return s._replace(route=expected_route(s.kind, s.D, s.Di, s.aw, s.cw, forced16, b3=True))


def b3_nets(s, forced16=False):
    """(the actor runs a B3 kernel, the critic does)."""
    return b3_net(okind(s.kind), s.aw, s.D, s.Di, forced16), b3_net("critic", s.cw, s.D, 0, forced16)


def b3_kernel_class(s, forced16=False):
    """kernel_class under the variant, and which of the two nets is B3."""
    k = okind(s.kind)
    route = expected_route(s.kind, s.D, s.Di, s.aw, s.cw, forced16, b3=True)
    return (route, s.aw, s.cw, k, first_layer_class(route[0], k, s.D), first_layer_class(route[1], "critic", s.D),
            b3_nets(s, forced16))


def b3_shape_cases(width=None):
    """The variable alone, B = 37.  Width 256: plain D 1..32 (one first-layer column block up to 16 floats, two above), modular
    Di 1 for every D the variant serves, Di 2 and 3, and (31, 3): a plant tower of 28 floats, the last one served.  Width 128:
    plain D 14..32 (below, the LDS-resident kernels serve both nets and nothing is B3) and the modular actor on 14 and 20 floats:
    the split pipeline (f32, float atomics) next to a B3 critic."""
    out = [b3_spec("plain", D, 0, 256, 37) for D in range(1, MAX_D + 1)]
    out += [b3_spec("modular", D, 1, 256, 37) for D in range(2, MAX_D + 1) if D - 1 <= B3_MAX_TOWER_256]
    out += [b3_spec("modular", D, Di, 256, 37) for D, Di in ((4, 2), (7, 3), (31, 3))]
    out += [b3_spec("plain", D, 0, 128, 37) for D in range(14, MAX_D + 1)]
    out += [b3_spec("modular", D, 1, 128, 37) for D in (14, 20)]
    return [s for s in out if width in (None, s.aw)]


def b3_regime_cases():
    """The first member of every B3 kernel class of the shape list at the 16-tile family's batch regimes, and per (route, width)
    one batch of grid x 64 + 1 -- carried as CAP_B: the variant's LDS footprint decides the grid, so the batch is sized where
    pime_ppo_grid16 can be asked under the variable (resolve_cap)."""
    seen, out, capped = {}, [], set()
    for s in b3_shape_cases():
        seen.setdefault(b3_kernel_class(s), s)
    for cls, s in seen.items():
        out += [s._replace(B=B) for B in REGIME_B["16tile"]]
        if (cls[0], s.aw) not in capped:
            capped.add((cls[0], s.aw))
            out.append(s._replace(B=CAP_B))
    return out


def b3_mixed_cases():
    """A B3 actor next to an f32 LDS-resident critic, at width 256 and (a critic of width 64 has no B3 kernel) at width 128; both B3
    at different tile counts; an LDS-resident actor next to a B3 critic."""
    out = []
    for B in (37, 257):
        out += [b3_spec("plain", 9, 0, 256, B, cw=128), b3_spec("plain", 20, 0, 256, B, cw=128), b3_spec("modular", 5, 2, 128, B, cw=256),
                b3_spec("plain", 20, 0, 128, B, cw=64)]
    return out


def b3_forced16_cases():
    """Both variables, width 128 (width 64 has no B3 kernel): ppo16_kernel<8, ., true> on narrow observations and
    ppo16m_kernel<8, true> -- Di 1 and 3, and on (20, 1) its two-tile first layer (a plant tower of 19 floats) --, B 2 .. 65; the
    modular actor once next to a critic of width 64 (the f32 16-tile kernel), and its cap batch."""
    shapes = (("plain", 3, 0), ("plain", 20, 0), ("modular", 4, 1), ("modular", 7, 3), ("modular", 20, 1))
    out = [b3_spec(k, D, Di, 128, B, forced16=True) for k, D, Di in shapes for B in (2, 15, 17, 37, 63, 65)]
    out.append(b3_spec("modular", 4, 1, 128, 37, cw=64, forced16=True))   # ppo16m_kernel<8, true> next to an f32 critic (width 64)
    return out + [b3_spec("modular", 4, 1, 128, CAP_B, forced16=True)]


def b3_per_route_shapes(forced16=False):
    """One shape per (route, widths, actor kind, which nets are B3): the first of the lists of the process."""
    seen = {}
    for s in (b3_forced16_cases() if forced16 else b3_shape_cases() + b3_mixed_cases()):
        if s.B != CAP_B:
            seen.setdefault((s.route, s.aw, s.cw, okind(s.kind), b3_nets(s, forced16)), s)
    return list(seen.values())


def b3_property_cases(forced16=False):
    return [s._replace(B=B) for s in b3_per_route_shapes(forced16) for B in (293, 100)]


B3_LISTS = {   # name -> (forced16, list): what the children of the GPU tests are told to run
    "shapes256": (False, lambda: b3_shape_cases(256)),
    "shapes128": (False, lambda: b3_shape_cases(128)),
    "regimes": (False, b3_regime_cases),
    "mixed": (False, b3_mixed_cases),
    "forced16": (True, b3_forced16_cases),
}


def b3_gradient_specs():
    """[(spec, forced16)]: every vetted spec of the variant's lists that gradient_specs() does not already hold (the cap
    placeholders are resolved and vetted where the grid can be read)."""
    have, out = set(gradient_specs()), []
    for forced16, cases in ((False, b3_shape_cases() + b3_regime_cases() + b3_mixed_cases() + b3_property_cases()),
                            (True, b3_forced16_cases() + b3_property_cases(True))):
        for s in cases:
            if s.B != CAP_B and s not in have:
                have.add(s)
                out.append((s, forced16))
    return out


def cap_grids(s, forced16=False):
    """{net: workgroups pime_ppo_grid16 answers for an unbounded batch} of the spec's nets on the 16-tile family, in THIS
    process (host-only query; it follows the process's variables)."""
    import pime_amd.native as nt
    L = nt.lib()
    out = {}
    if s.route[0] == "16tile":
        out["actor"] = L.pime_ppo_grid16(nt.MLP_MODULAR_ACTOR if s.kind == "modular" else nt.MLP_PLAIN_ACTOR, 1 << 30, s.aw, s.D, s.Di)
    if s.route[1] == "16tile":
        out["critic"] = L.pime_ppo_grid16(nt.MLP_CRITIC, 1 << 30, s.cw, s.D, 0)
    assert out and min(out.values()) >= 1
    return out


def resolve_cap(s, forced16=False):
    """(the spec at B = largest grid x 64 + 1, the grids): every 16-tile net's workgroups take a second group."""
    grids = cap_grids(s, forced16)
    B = max(grids.values()) * 64 + 1
    assert all((B + 63) // 64 > g for g in grids.values()), "no workgroup of the 16-tile kernel takes a second group"
    return s._replace(B=B), grids


# --------------------------------------------------------------------------------------------------------------- generator
# Three gradient tensors have ONE element (the two head biases and a_std_log): a sum of B terms of either sign, which in about one
# case of 500 cancels to a thousandth of its terms -- float32 then keeps 1e-3 of it, and no kernel could meet the bar on it.  That
# is a property of the draw, so such a case draws again: `build` takes the first salt of 0, 1, 2, ... at which the float32 oracle
# stays within F32_STABILITY / 4 of the float64 one (a quarter: the choice must not depend on the BLAS of the machine that makes
# it), and records it.  The CPU test holds every case to F32_STABILITY itself and to a salt of at most MAX_SALT.
MAX_SALT = 3


def _linear(rng, n_out, n_in):
    k = 1.0 / np.sqrt(n_in)
    return rng.uniform(-k, k, (n_out, n_in)), rng.uniform(-k, k, n_out)


def _rescale(p, name, z, std=1.0):
    k = std / z.std()
    p[name + ".weight"] *= k
    p[name + ".bias"] *= k


def make_nets(kind, D, Di, aw, cw, seed):
    """(actor, critic) state dicts, float32, at the scales of the module docstring (set on 256 probe rows)."""
    rng = np.random.RandomState([seed, aw, cw, D, Di, 29])
    probe = rng.uniform(-1.5, 1.5, (256, D))
    cri = {}
    for name, (o, i) in zip(P.CRITIC_LAYERS, ((cw, D), (cw, cw), (cw, cw), (1, cw))):
        cri[name + ".weight"], cri[name + ".bias"] = _linear(rng, o, i)
    for i, name in enumerate(P.CRITIC_LAYERS[:3]):
        _rescale(cri, name, P.critic_forward(cri, probe)[1][i])
    _rescale(cri, "net.6", P.critic_forward(cri, probe)[0])
    act = {"a_std_log": np.full((1, 1), A_STD_LOG)}
    if kind == "modular":
        half = aw // 2
        shapes = ((aw, D - Di), (half, aw), (aw, Di), (half, aw), (aw, 2 * half), (1, aw))
        for name, (o, i) in zip(P.MODULAR_LAYERS, shapes):
            act[name + ".weight"], act[name + ".bias"] = _linear(rng, o, i)
        xo, xi = probe[:, :D - Di], probe[:, D - Di:]
        _rescale(act, "other_net.0", P._lin(act, "other_net.0", xo))
        _rescale(act, "other_net.2", P._lin(act, "other_net.2", np.tanh(P._lin(act, "other_net.0", xo))))
        _rescale(act, "integrator_net.0", P._lin(act, "integrator_net.0", xi))
        _rescale(act, "integrator_net.2", P._lin(act, "integrator_net.2", np.tanh(P._lin(act, "integrator_net.0", xi))))
        cat = P.actor_forward(act, "modular", Di, probe)[1][6]
        _rescale(act, "net.0", P._lin(act, "net.0", cat))
        _rescale(act, "net.2", P.actor_forward(act, "modular", Di, probe)[0])
    else:
        for name, (o, i) in zip(P.PLAIN_LAYERS, ((aw, D), (aw, aw), (aw, aw), (1, aw))):
            act[name + ".weight"], act[name + ".bias"] = _linear(rng, o, i)
        for i, name in enumerate(P.PLAIN_LAYERS[:3]):
            _rescale(act, name, P._lin(act, name, P.actor_forward(act, "plain", 0, probe)[1][i]))
        _rescale(act, "net.6", P.actor_forward(act, "plain", 0, probe)[0])
    return tuple({k: v.astype(np.float32) for k, v in p.items()} for p in (act, cri))


def okind(kind):
    """The oracle's name of a spec's actor kind."""
    return "modular" if kind == "modular" else "plain"


def _draw_rows(rng, nets, s, rows):
    """Table rows `rows` (their combination is row mod 10): (state, action, logprob, adv, r_sum), float32."""
    act, cri = nets
    n = len(rows)
    cat, branch = (rows % 10) % 5, (rows % 10) // 5
    state = rng.uniform(-1.5, 1.5, (n, s.D)).astype(np.float32)
    mean, _ = P.actor_forward(act, okind(s.kind), s.Di, state)
    action = (mean + np.exp(A_STD_LOG) * np.clip(rng.standard_normal(n), -2.5, 2.5)).astype(np.float32)
    sign = np.where(np.isin(cat, (1, 4)), 1.0, np.where(cat == 0, rng.choice([-1.0, 1.0], n), -1.0))
    mag = 0.1 + np.abs(rng.standard_normal(n))
    mag[rows == N_ROWS - 1] = max(1.0, 10.0 * np.sqrt(s.B) / 256)   # the last sample of a large batch: see the module docstring
    adv = (sign * mag).astype(np.float32)
    ratio = np.where(cat == 0, rng.uniform(0.85, 1.15, n), np.where(cat <= 2, rng.uniform(1.25, 1.8, n), rng.uniform(0.45, 0.75, n)))
    logprob = (P.logprob(act, okind(s.kind), s.Di, state, action) - np.log(ratio)).astype(np.float32)
    off = np.where(branch == 0, rng.uniform(0.1, 0.9, n), rng.uniform(1.1, 3.0, n)) * rng.choice([-1.0, 1.0], n)
    r_sum = (P.critic_forward(cri, state)[0] + off).astype(np.float32)
    return state, action, logprob, adv, r_sum


def categories(case, d=None, ratio=None):
    """(ratio category, SmoothL1 branch) index of every sample, from the oracle's own ratio and v - r_sum (not from the generator's
    intent): what the share conditions are asserted on."""
    adv = case.table[3][case.idx]
    ratio = case.mid["ratio"] if ratio is None else ratio
    d = case.mid["d"] if d is None else d
    hi, lo = ratio > 1 + RATIO_CLIP, ratio < 1 - RATIO_CLIP
    cat = np.where(hi & (adv > 0), 1, np.where(hi, 2, np.where(lo & (adv < 0), 3, np.where(lo, 4, 0))))
    return cat, (np.abs(d) >= 1).astype(int)


Case = collections.namedtuple("Case", "spec nets table idx redrawn rounds mid salt")


def batch_of(case, subset=None):
    idx = case.idx if subset is None else case.idx[subset]
    return tuple(t[idx] for t in case.table)


def _pick(rng, pos):
    """A table row of combination pos mod 10, away from the two rows that positions 0 and B - 1 name."""
    return 10 * rng.randint(1, N_ROWS // 10 - 1, size=np.shape(pos)) + np.asarray(pos) % 10


def f32_distance(case):
    """Largest |float32 oracle - float64 oracle| over the gradient tensors, as a share of each tensor's largest entry."""
    lo = reference(case, dt=np.float32)
    return max(float(np.abs(lo[net][k].astype(np.float64) - want).max() / np.abs(want).max())
               for net in ("ga", "gc") for k, want in case.mid[net].items())


@functools.lru_cache(maxsize=None)
def build(s):
    """The case of a spec: `_build` at the first salt whose draw is well conditioned in float32 (vetted cases; see MAX_SALT)."""
    for salt in range(MAX_SALT + 1):
        case = _build(s, salt)
        if not s.vet or f32_distance(case) <= F32_STABILITY / 4:
            break
    return case


def _build(s, salt):
    """The case of a spec: nets, the trajectory table (state [N_ROWS, D], action, logprob, adv, r_sum [N_ROWS]) and the index list
    [B].  With s.vet, table rows whose kink margin is below DELTA are drawn again (same combination) until none is left;
    Case.redrawn counts the rows of the first pass that had to go.  The margin of a ReLU layer is relative to the layer's largest
    |pre-activation|, and a batch's largest is at most the table's: a row that clears DELTA against the table's scales clears it
    in every batch drawn from the table, so the index list needs no redraw of its own -- Case.mid["margin"] holds the batch's own
    margins, which the CPU test asserts.  (Redrawing per batch instead would trip the cap by chance alone: a width-256 critic
    has 768 ReLU units per sample, 3.4 % of the samples sit within DELTA of one, and a 37-sample case may redraw three.)
    Case.mid: the float64 oracle on the final inputs (with "margin", and "d" = v - r_sum)."""
    seed = (s.aw * 1000003 + s.cw * 50021 + s.D * 10007 + s.Di * 1009 + s.B * 101 + (s.kind == "ppo")) % (2 ** 31)
    rng = np.random.RandomState([seed, salt])
    nets = make_nets(okind(s.kind), s.D, s.Di, s.aw, s.cw, seed)
    table = [np.array(t) for t in _draw_rows(rng, nets, s, np.arange(N_ROWS))]
    idx = _pick(rng, np.arange(s.B)).astype(np.int64)
    fixed = {0: 0, s.B - 1: N_ROWS - 1}
    for pos, r in fixed.items():
        idx[pos] = r
    twin = (1, 11) if s.B >= 13 else (1, 2) if s.B >= 4 else ()   # one guaranteed repeat: the second position names the first one's row
    if twin:
        idx[twin[1]] = idx[twin[0]]
    act, cri = nets
    ok = okind(s.kind)
    rounds = redrawn = 0
    while s.vet:   # the TABLE is vetted, against its own scales: see below
        m, scales, _, _ = P.sample_margins(act, cri, ok, s.Di, table, RATIO_CLIP)
        bad = np.flatnonzero(m < DELTA)
        if bad.size == 0:
            break
        redrawn += bad.size if rounds == 0 else 0
        while bad.size:   # the redrawn rows alone, against the table's scales, until they are clear; then the whole table again
            rounds += 1
            assert rounds < 200, "redraw does not converge"
            for t, new in zip(table, _draw_rows(rng, nets, s, bad)):
                t[bad] = new
            m = P.sample_margins(act, cri, ok, s.Di, [t[bad] for t in table], RATIO_CLIP, scales)[0]
            bad = bad[m < 2 * DELTA]   # (twice: the whole-table pass that follows may move the scales a little)
    for a in table + [idx]:
        a.setflags(write=False)
    case = Case(s, nets, tuple(table), idx, redrawn, rounds, None, salt)
    mid = reference(case, margins=s.vet)
    return case._replace(mid=mid)


def reference(case, dt=np.float64, mutant=None, margins=False, light=False):
    """ppo_oracle.gradients on the case's minibatch at the cases' clip and entropy weight; "d" = v - r_sum added."""
    s = case.spec
    act, cri = case.nets
    out = P.gradients(act, cri, okind(s.kind), s.Di, batch_of(case), RATIO_CLIP, LAMBDA_ENTROPY, dt, mutant, margins, light)
    if mutant is None and not light:
        b = batch_of(case)
        out["d"] = P.critic_forward(cri, b[0])[0] - b[4].astype(np.float64)
    return out


def mutant_reach(case, mutant):
    """Largest |mutant's gradient - oracle's| / max|oracle's| over the gradient tensors; the head gradients and a_std_log first
    (a lower bound of the reach, cheaper), every tensor if that does not already exceed MUTATION_MARGIN x BAR."""
    reach = 0.0
    for light in (True, False):
        got = reference(case, mutant=mutant, light=light)
        for net in ("ga", "gc"):
            want = case.mid[net]
            for k, g in got[net].items():
                reach = max(reach, float(np.abs(g - want[k].reshape(g.shape)).max() / np.abs(want[k]).max()))
        if reach > MUTATION_MARGIN * BAR:
            break
    return reach
