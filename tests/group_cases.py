"""What tests/test_param_groups.py (GPU) and tests/test_param_groups_cpu.py share about the raw glowtts_adam_noam_groups kernel: the
inputs, the option sets, the fp64 reference of one group's update, the kernel's own sequence of fp32 operations in numpy, and the
bounds.

Inputs: ema_cases.adam_ema_data (the recipe of tests/test_train_tail.py::_adam_data plus e; `dead` elements with g = m = v = 0 and,
of those, `pad` elements with p = e = 0 as well: what the flat buffers' padding holds).

Reference: one update in fp64 with the semantics of torch.optim.Adam(weight_decay=, decoupled_weight_decay=) of the installed
torch (tests/test_param_groups_cpu.py checks `group_ref` against torch.optim.Adam itself, in fp64, for each decay form):
    rate   = rate_t * lr_scale                    rate_t: the imposed rate, or noam_lr(s), shared by the groups of a launch
    L2        : g' = g + wd p goes into the moments;  decoupled : p <- p (1 - rate wd) first;  wd = 0 : neither
    m' = b1 m + (1 - b1) g',  v' = b2 v + (1 - b2) g'^2,  upd = rate / (1 - b1^t) * m' / (sqrt(v') / sqrt(1 - b2^t) + eps),  p' = p - upd
Hyper-parameters and options are the fp32 values the C ABI receives.

Bounds, per element, in units of u = 2**-24 of the magnitudes tests/test_train_tail.py::test_adam_one_update_raw uses, the L2 form's
gradient counted with its decay term:
    m : |b1 m| + |(1 - b1) g| (+ |(1 - b1) wd p| for L2)        v : |v'|        p : |p| + |upd|
The kernel's sequence of fp32 operations (`group_np32`) evaluated with numpy on the CPU against fp64 on these inputs — sizes
MEASURE_SIZES, both STATES, every option set of a form — is off by at most (MEASURED; test_param_groups_cpu.py re-measures them and
fails if they moved):
    form        m        v        p
    plain       1.95 u   2.54 u    9.62 u
    l2          2.85 u   3.69 u   12.58 u
    decoupled   1.95 u   2.54 u    9.61 u
and the GPU bound is 4 x the worst figure of a form, rounded up to a power of two (BOUNDS): 8 / 16 / 64 u, 16 / 16 / 64 u, 8 / 16 / 64 u.
The p figure grows with the number of elements looked at (2.3 u over the sizes up to 4224 alone): where b1 m and (1 - b1) g cancel, a
few u of their magnitudes is a large relative error of m', and the scale |p| + |upd| does not see it (tests/test_train_tail.py says the
same of its own 9.2 u).  So the sizes measured are the sizes the GPU test runs, the largest included.
(lr_scale = 0.1 and lr_scale = 0 are "plain" with another rate; with lr_scale = 0 p must come out bit for bit.)"""
import math

import numpy as np
import torch

from ema_cases import B1, B2, DIM, EPS, LR, PAD, U, WARMUP, adam_ema_data, units  # noqa: F401  (re-exported to the two test files)

# (t, noam step, state[2], imposed rate): an imposed rate (the largest steps of test_train_tail's states), and the schedule's own
STATES = [(4.0, 2.0, 123.0, 0.0241), (7.0, 123456.0, 123.0, 0.0)]
MEASURE_SIZES = [5, 192, 196, 512, 1023, 4224, 2 ** 21 + 192]      # the n of every shape the GPU test runs

# name -> (lr_scale, weight_decay, decoupled, frozen) and the decay form whose bound applies
OPTIONS = {
    "default": (1.0, 0.0, 0, 0),
    "scale0.1": (0.1, 0.0, 0, 0),
    "scale0": (0.0, 0.0, 0, 0),
    "l2": (1.0, 0.01, 0, 0),
    "decoupled": (1.0, 0.01, 1, 0),
    "scale0.1+l2": (0.1, 0.01, 0, 0),
    "scale0.1+decoupled": (0.1, 0.01, 1, 0),
    "frozen": (1.0, 0.0, 0, 1),
    "frozen+decay": (0.5, 0.01, 1, 1),            # a frozen group's other options mean nothing
}
FROZEN = {name for name, o in OPTIONS.items() if o[3]}


def form_of(name):
    scale, wd, decoupled, _ = OPTIONS[name]
    return "plain" if wd == 0.0 else ("decoupled" if decoupled else "l2")


MEASURED = {"plain": (1.95, 2.54, 9.62), "l2": (2.85, 3.69, 12.58), "decoupled": (1.95, 2.54, 9.61)}      # m, v, p in u


def bound_from(figure):
    """4 x the figure, rounded up to a power of two."""
    return 2.0 ** math.ceil(math.log2(4.0 * figure))


BOUNDS = {form: tuple(bound_from(f) for f in figs) for form, figs in MEASURED.items()}


def f32(x):
    """The value a C `float` argument of the ABI holds."""
    return float(np.float32(x))


def noam_lr(s, dim=DIM, warmup=WARMUP, lr=LR):
    """reference optimize.py:32-41 in fp64, lr as the fp32 the ABI receives."""
    return f32(lr) * dim ** -0.5 * min(s ** -0.5, s * warmup ** -1.5)


def rate_of(state):
    """The shared rate of a launch in fp64: the imposed one if there is one, else the schedule's."""
    return float(np.float32(state[3])) if state[3] > 0 else noam_lr(state[1])


def group_ref(p, g, m, v, state, option, b1=B1, b2=B2, eps=EPS):
    """fp64: (p', m', v', upd, m_scale) of one group's elements; see the module docstring."""
    scale, wd, decoupled, _ = (f32(x) for x in option)
    b1, b2, eps = f32(b1), f32(b2), f32(eps)
    p, g, m, v = (x.double() for x in (p, g, m, v))
    t = state[0]
    rate = rate_of(state) * scale
    m_scale = (b1 * m).abs() + ((1 - b1) * g).abs()
    if wd != 0.0 and decoupled:
        p = p * (1 - rate * wd)
    elif wd != 0.0:
        m_scale = m_scale + ((1 - b1) * wd * p).abs()
        g = g + wd * p
    m1 = b1 * m + (1 - b1) * g
    v1 = b2 * v + (1 - b2) * g * g
    upd = rate / (1 - b1 ** t) * (m1 / (v1.sqrt() / math.sqrt(1 - b2 ** t) + eps))
    return p - upd, m1, v1, upd, m_scale


def group_np32(p, g, m, v, state, option, b1=B1, b2=B2, eps=EPS):
    """(p', m', v') by the kernel's sequence of fp32 operations in numpy (csrc/train_ops.hip: adam_update with a GroupTable): the
    shared rate rounded to fp32, rate_k = fl32(rate * lr_scale), step_size and the decoupled factor formed in fp64 and rounded
    once, weight_decay == 0 taking the plain expressions.  No contraction (the library is built with -ffp-contract=off)."""
    f = np.float32
    scale, wd, decoupled, _ = option
    p, g, m, v = (x.numpy().astype(f) for x in (p, g, m, v))
    t = float(f(state[0]))
    b1, b2, eps = f(b1), f(b2), f(eps)
    rate = f(f(rate_of(state)) * f(scale))
    step_size = f(float(rate) / (1.0 - float(b1) ** t))
    inv_sqrt_bc2 = f(1.0 / np.sqrt(1.0 - float(b2) ** t))
    if f(wd) != 0 and decoupled:
        p = p * f(1.0 - float(rate) * float(f(wd)))
    elif f(wd) != 0:
        g = g + f(wd) * p
    m1 = b1 * m + (f(1.0) - b1) * g
    v1 = b2 * v + (f(1.0) - b2) * g * g
    denom = np.sqrt(v1) * inv_sqrt_bc2 + eps
    return tuple(torch.from_numpy(x) for x in (p - step_size * (m1 / denom), m1, v1))


def figures(got_p, got_m, got_v, p, g, m, v, state, option):
    """(m, v, p) figures in u of what a kernel (or group_np32) gave for one group against group_ref."""
    want_p, want_m, want_v, upd, m_scale = group_ref(p, g, m, v, state, option)
    return (units(got_m, want_m, m_scale), units(got_v, want_v, want_v.abs()), units(got_p, want_p, p.double().abs() + upd.abs()))


def measure():
    """form -> worst (m, v, p) figures of group_np32 over MEASURE_SIZES x STATES x the live option sets."""
    worst = {}
    for n in MEASURE_SIZES:
        p, g, m, v = adam_ema_data(n)[:4]
        for state in STATES:
            for name, option in OPTIONS.items():
                if name in FROZEN:
                    continue
                figs = figures(*group_np32(p, g, m, v, state, option), p, g, m, v, state, option)
                form = form_of(name)
                worst[form] = tuple(max(a, b) for a, b in zip(worst.get(form, (0.0, 0.0, 0.0)), figs))
    return worst
