"""Test helper: the case table and the float64 reference of the fused MLP forward / pack sweep (tests/test_gpu_mlp_sweep.py;
vetted on the CPU by tests/test_mlp_cases_cpu.py) -- TEST INFRASTRUCTURE ONLY.

Reference: plain numpy, written from this package's modules (elegantrl/net.py, elegantrl/net_residual.py), not from the kernels:
    critic          CriticAdv.forward / the TD3 Actor before its tanh   D -> md ReLU -> md ReLU -> md ReLU -> 1
    plain_actor     ActorPPO / ActorResidualPPO.mean                    D -> md Tanh -> md Tanh -> md Tanh -> 1
    modular_actor   ActorResidualIntegratorModularPPO.mean              x[:, :Do] -> md Tanh -> md/2 Tanh  |  x[:, Do:] -> md Tanh -> md/2
                                                                        Tanh, concatenated in that order -> md Tanh -> 1  (Do = D - Di)
    sac_actor       ActorSAC: net_a_avg(net_state(x)), before its tanh  D -> md ReLU -> md Hardswish -> md Hardswish -> 1
                                                                        (tests/sac_oracle.py: actor_forward, key "avg")
It runs in the dtype of its operands: float64 is the reference, float32 (numpy's own summation order) shows that a case is not
ill-conditioned for float32.

Weights: seeded standard_normal * 1.5 / sqrt(fan_in), biases standard_normal * 0.3, head rows * 5 (ActorSAC: both head rows, drawn
separately), rounded to float32 -- the float64 reference reads the same float32 values the kernels do.
Rows: M = 97 (three full 32-row tiles + a ragged one; one full 64-row group + a ragged one) of tank-scaled observations as
tests/test_gpu_mlp16.py: check_forward draws them; row 0 is all zeros, row 1 is scaled by 1e-3; the two tanh kinds also get row 2 at
+-1e4 (random signs) and row 3 at -3e30, where tanh sits on its ends.  The ReLU and Hardswish kinds get no extreme rows: their error
scales with the input.
Bar (the project's standing one for both kernel families): |got - want| <= 3e-5 |want| + 3e-5 max(1, max |want|) per case.
A case's draw is kept if the float32 forward uses at most a tenth of the bar; otherwise the next salt is drawn (a hidden unit of the
+-1e4 row can land inside tanh's bend, where a float32 pre-activation of that size carries an error of 1e-3).

Shapes: plain kinds every D in 1..32; the modular actor MODULAR_SHAPES (both towers at width 1, every padding D % 4 of either tower,
the largest first-layer images).  Widths 64 / 128 / 256 (ActorSAC: 64 / 128).

Kernel instantiations (csrc/mlp_mfma.hip, csrc/mlp16.hip), by test id:
    {critic,plain_actor,modular_actor,sac_actor}-{64,128}-D*   mlp_forward_kernel<{2,4}, KIND>                    8   mlp_pack_kernel
    {critic,plain_actor}-256-D*                                mlp16_forward_kernel<16, {0,1}>                    2   pack16_kernel
    modular_actor-256-D*-Di*                                   mlp16m_forward_kernel<16>                          1   pack16m_kernel
    forced16-{critic,plain_actor}-{64,128}-D*                  mlp16_forward_kernel<{4,8}, {0,1}> (PIME_MLP16)    4   pack16_kernel
15 forward kernels and 3 pack kernels."""
import collections
import functools

import numpy as np

import sac_oracle as S

BAR = 3e-5
F32_SHARE = 0.1           # the float32 forward may use this much of the bar
MUTATION_MARGIN = 10.0    # every mutant moves some row by this many bars
MAX_SALT = 8
M = 97
MAX_D = 32
WIDTHS = (64, 128, 256)
QUERY_WIDTHS = (32, 64, 128, 256, 512)
KINDS = ("critic", "plain_actor", "modular_actor", "sac_actor")
TANH_KINDS = ("plain_actor", "modular_actor")
MODULAR_SHAPES = ((2, 1), (3, 1), (3, 2), (4, 1), (5, 4), (6, 3), (9, 5), (29, 1), (30, 15), (32, 1), (32, 16), (32, 31))
FORCED_D = (1, 2, 3, 5, 29, 32)
LAYERS = {
    "critic": ("net.0", "net.2", "net.4", "net.6"),
    "plain_actor": ("net.0", "net.2", "net.4", "net.6"),
    "modular_actor": ("other_net.0", "other_net.2", "integrator_net.0", "integrator_net.2", "net.0", "net.2"),
    "sac_actor": ("net_state.0", "net_state.2", "net_state.4", "net_a_avg", "net_a_std"),
}
HEADS = ("net.6", "net_a_avg", "net_a_std")   # and the modular actor's net.2

Spec = collections.namedtuple("Spec", "kind md D Di")
Case = collections.namedtuple("Case", "spec params x want salt f32_share")


# ---- the served set -----------------------------------------------------------------------------------------------------------
def served(kind, md, D, Di):
    """What pime_mlp_packed_floats answers with a size (include/pime_hip.h)."""
    if not 1 <= D <= MAX_D:
        return False
    if kind == "modular_actor":
        return md in (64, 128, 256) and 1 <= Di < D
    if kind == "sac_actor":
        return md in (64, 128)
    return md in (64, 128, 256)


# ---- the case table -------------------------------------------------------------------------------------------------------------
def forward_specs():
    out = []
    for kind in KINDS:
        for md in WIDTHS:
            if kind == "modular_actor":
                out += [Spec(kind, md, D, Di) for D, Di in MODULAR_SHAPES]
            elif served(kind, md, 1, 0):
                out += [Spec(kind, md, D, 0) for D in range(1, MAX_D + 1)]
    return out


def forced16_specs():
    """What PIME_MLP16 routes to the 16-tile family instead: the plain nets of width 64 / 128."""
    return [Spec(kind, md, D, 0) for kind in ("critic", "plain_actor") for md in (64, 128) for D in FORCED_D]


def spec_id(s, forced16=False):
    return ("forced16-" if forced16 else "") + f"{s.kind}-{s.md}-D{s.D}" + (f"-Di{s.Di}" if s.kind == "modular_actor" else "")


def family16(s, forced16=False):
    if s.kind == "sac_actor":
        return False
    if s.kind == "modular_actor" or s.md == 256:
        return s.md == 256
    return forced16


def forward_kernel(s, forced16=False):
    if not family16(s, forced16):
        return f"mlp_forward_kernel<{s.md // 32}, {s.kind}>"
    if s.kind == "modular_actor":
        return "mlp16m_forward_kernel<16>"
    return f"mlp16_forward_kernel<{s.md // 16}, {0 if s.kind == 'critic' else 1}>"


def pack_kernel(s, forced16=False):
    if not family16(s, forced16):
        return "mlp_pack_kernel"
    return "pack16m_kernel" if s.kind == "modular_actor" else "pack16_kernel"


def table():
    """test id -> (forward kernel, pack kernel)"""
    t = {spec_id(s): (forward_kernel(s), pack_kernel(s)) for s in forward_specs()}
    t.update({spec_id(s, True): (forward_kernel(s, True), pack_kernel(s, True)) for s in forced16_specs()})
    return t


# ---- weights and rows -----------------------------------------------------------------------------------------------------------
def layer_shapes(s):
    """(name, out, in) in the order pime_mlp_pack takes the tensors (ops._PARAM_ORDER)."""
    md, D, Di = s.md, s.D, s.Di
    if s.kind == "modular_actor":
        dims = ((md, D - Di), (md // 2, md), (md, Di), (md // 2, md), (md, md), (1, md))
    elif s.kind == "sac_actor":
        dims = ((md, D), (md, md), (md, md), (1, md), (1, md))
    else:
        dims = ((md, D), (md, md), (md, md), (1, md))
    return [(name, o, i) for name, (o, i) in zip(LAYERS[s.kind], dims)]


def _is_head(s, name):
    return name in HEADS or (s.kind == "modular_actor" and name == "net.2")


def draw(s, salt=0):
    rng = np.random.RandomState(((KINDS.index(s.kind) * 4 + WIDTHS.index(s.md)) * 64 + s.D) * 64 + s.Di + 1000003 * salt)
    p = {}
    for name, o, i in layer_shapes(s):
        w = rng.standard_normal((o, i)) * 1.5 / np.sqrt(i)
        p[name + ".weight"] = (w * 5.0 if _is_head(s, name) else w).astype(np.float32)
        p[name + ".bias"] = (rng.standard_normal(o) * 0.3).astype(np.float32)
    D = s.D
    x = (rng.standard_normal((M, D)) * np.array(([3., 3., 8., 1.] * 8)[:D]) + np.array(([7., 7., 0., 0.] * 8)[:D])).astype(np.float32)
    x[0] = 0.0
    x[1] *= np.float32(1e-3)
    if s.kind in TANH_KINDS:
        x[2] = np.where(rng.uniform(size=D) < 0.5, -1e4, 1e4)
        x[3] = -3e30
    return p, x


# ---- the reference --------------------------------------------------------------------------------------------------------------
MUTANTS_INPUT = ("last_column_dropped", "columns_swapped")
MUTANTS_MODULAR = ("boundary_moved", "towers_swapped")
MUTANTS_NET = ("weight_transposed", "bias_swapped", "relu_tanh")
MUTANTS_SAC = ("relu_for_hardswish_2", "relu_for_hardswish_3", "std_head")
MUTANTS = MUTANTS_INPUT + MUTANTS_MODULAR + MUTANTS_NET + MUTANTS_SAC
SQUARE = {"critic": "net.2", "plain_actor": "net.2", "modular_actor": "net.0", "sac_actor": "net_state.2"}   # an md x md layer
LAST_HIDDEN = {"critic": "net.4", "plain_actor": "net.4", "modular_actor": "net.0", "sac_actor": "net_state.4"}


def mutants_of(s):
    out = ["last_column_dropped"] + (["columns_swapped"] if s.D >= 2 else [])
    if s.kind == "modular_actor":
        out += (["boundary_moved"] if s.D >= 3 else []) + ["towers_swapped"]
    out += ["weight_transposed", "bias_swapped"]
    out += list(MUTANTS_SAC) if s.kind == "sac_actor" else ["relu_tanh"]   # (ActorSAC's forward is tests/sac_oracle.py's, with its mutants)
    return out


def _relu(v):
    return np.maximum(v, 0)


def _lin(p, name, h):
    return h @ p[name + ".weight"].T + p[name + ".bias"]


def forward(kind, p, x, Di=0, mutant=None):
    """The scalar head [M] of the net `kind` with parameters p on the rows x, in the dtype of p and x.  `mutant` changes ONE thing."""
    assert mutant is None or mutant in MUTANTS
    dt = x.dtype
    assert all(v.dtype == dt for v in p.values())
    D = x.shape[1]
    if mutant == "last_column_dropped":
        x = x.copy()
        x[:, -1] = 0
    elif mutant == "columns_swapped":
        x = x.copy()
        x[:, [0, D - 1]] = x[:, [D - 1, 0]]
    elif mutant == "weight_transposed":
        p = dict(p)
        p[SQUARE[kind] + ".weight"] = np.ascontiguousarray(p[SQUARE[kind] + ".weight"].T)
    elif mutant == "bias_swapped":   # the two features whose biases differ most
        p = dict(p)
        b = p[LAST_HIDDEN[kind] + ".bias"].copy()
        i, j = int(np.argmax(b)), int(np.argmin(b))
        b[[i, j]] = b[[j, i]]
        p[LAST_HIDDEN[kind] + ".bias"] = b
    if kind == "sac_actor":
        f = S.actor_forward(p, x, mutant=mutant if mutant in S.MUTANTS else None)
        return (f["raw"] if mutant == "std_head" else f["avg"])[:, 0]
    act = (np.tanh if kind == "critic" else _relu) if mutant == "relu_tanh" else (_relu if kind == "critic" else np.tanh)
    if kind in ("critic", "plain_actor"):
        h = act(_lin(p, "net.0", x))
        h = act(_lin(p, "net.2", h))
        h = act(_lin(p, "net.4", h))
        return _lin(p, "net.6", h)[:, 0]
    assert kind == "modular_actor" and 1 <= Di < D
    Do = D - Di
    xo, xi = x[:, :Do], x[:, Do:]
    if mutant == "boundary_moved":   # the towers split the row one column off (towards the wider tower); what falls outside is zero
        b = Do - 1 if Do >= 2 else Do + 1
        xo, xi = np.zeros_like(xo), np.zeros_like(xi)
        xo[:, :min(b, Do)] = x[:, :min(b, Do)]
        xi[:, :min(Di, D - b)] = x[:, b:b + Di]
    plant = act(_lin(p, "other_net.2", act(_lin(p, "other_net.0", xo))))
    integ = act(_lin(p, "integrator_net.2", act(_lin(p, "integrator_net.0", xi))))
    cat = np.concatenate([integ, plant] if mutant == "towers_swapped" else [plant, integ], axis=-1)
    return _lin(p, "net.2", act(_lin(p, "net.0", cat)))[:, 0]


def cast(p, dt):
    return {k: np.asarray(v, dtype=dt) for k, v in p.items()}


def reference(s, p, x, dt=np.float64, mutant=None):
    return forward(s.kind, cast(p, dt), np.asarray(x, dtype=dt), s.Di, mutant)


def bar(want):
    want = np.asarray(want, dtype=np.float64)
    return BAR * np.abs(want) + BAR * max(1.0, float(np.abs(want).max()))


def share(got, want):
    """The largest used share of the bar over the rows (inf for a row that is not finite)."""
    got = np.asarray(got, dtype=np.float64)
    if not np.isfinite(got).all():
        return float("inf")
    return float((np.abs(got - want) / bar(want)).max())


@functools.lru_cache(maxsize=12)
def build(s):
    """The case of a spec: float32 parameters and rows, the float64 reference, and how the draw was found."""
    for salt in range(MAX_SALT + 1):
        p, x = draw(s, salt)
        want = reference(s, p, x)
        used = share(reference(s, p, x, dt=np.float32), want)
        if used <= F32_SHARE:
            break
    for a in list(p.values()) + [x, want]:
        a.setflags(write=False)
    return Case(s, p, x, want, salt, used)


def mutant_reach(case, mutant):
    """By how many bars the mutant moves the row it moves most."""
    return share(reference(case.spec, case.params, case.x, mutant=mutant), case.want)


# ---- the images (include/pime_hip.h; csrc/mlp_device.hpp: mlp_layout, csrc/mlp16.hip: layout16 / layout16m) -------------------------
def image_padding(s, forced16=False):
    """(zeros, unwritten) floats of a packed image that hold no parameter.  32x32x2 images: every segment is whole but the scalar head
    bias, which sits in 4 floats (3 unwritten per head row).  16-tile images: the first layers' columns are padded with ZEROS to a
    multiple of 4 per tower (0 x garbage must stay 0), and the head bias sits in 4 floats, the other 3 written as zeros."""
    if not family16(s, forced16):
        return 0, 3 * (2 if s.kind == "sac_actor" else 1)
    towers = (s.D - s.Di, s.Di) if s.kind == "modular_actor" else (s.D,)
    return sum((-d) % 4 for d in towers) * s.md + 3, 0


LDS_LIMIT = 160 * 1024


def lds16_forward_bytes(s):
    """The dynamic LDS the 16-tile forward kernels ask for (csrc/mlp16.hip: lds16 / lds16m with grad = false): the first layers' images
    (4 columns per k-step, padded per tower), the bias / head vectors, 48 floats of wave sums, and three slice buffers of the streamed
    layers (one buffer of 16 k-steps at width 64; 8 k-steps x width / 64 quads x 256 floats each from width 128 on)."""
    md, T = s.md, s.md // 16
    towers = (s.D - s.Di, s.Di) if s.kind == "modular_actor" else (s.D,)
    first = sum((d + 3) // 4 for d in towers) * T * 64
    vectors = (md + md // 2) * 2 + md + md + 4 if s.kind == "modular_actor" else 4 * md + 4
    region = 16 * 256 if T == 4 else 3 * 8 * (T // 4) * 256
    return 4 * (first + vectors + 48 + region)
