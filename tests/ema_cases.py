"""What tests/test_ema.py (GPU) and tests/test_ema_cpu.py share about the raw glowtts_adam_noam_ema kernel: the inputs, the cases,
the fp64 reference of the averaging step, the kernel's own sequence of fp32 operations in numpy, and the bound."""
import functools

import numpy as np
import torch

U = 2.0 ** -24
PAD = 8
LR, DIM, WARMUP = 0.01, 192.0, 4000.0
B1, B2, EPS = 0.9, 0.98, 1e-9
STATE = (4.0, 2.0, 123.0, 0.0241)            # t != step_num, a pending imposed rate: the largest steps of test_train_tail's states
SIZES = [1, 5, 1023, 4099, 600001, 2 ** 21 + 4]

# (ema_rate, ema_warm, k = averaged updates so far) -> the weight a of the new parameters
#   plain: a = ema_rate;  warm-up: a = max(ema_rate, 9 / (10 + k)) = 0.9, 0.6 and 8.9991e-5 (the formula, not the 1e-5 floor)
EMA_CASES = [(1e-4, 0, 0), (0.1, 0, 3), (1e-5, 1, 0), (1e-5, 1, 5), (1e-5, 1, 10 ** 5)]

# |e_new - (e + a (p' - e))| <= E_BOUND u (|e| + |p'|) per element, p' the updated parameter, a as the kernel rounds it.
# The kernel's sequence — d = fl(p' - e), fl(a d), fl(e + .) — evaluated with numpy in fp32 on the CPU against fp64 on these
# inputs is at most 2.37 u off (a = 0.9; 1.00 u for the two small weights; test_ema_cpu.py measures it); 4 x that, rounded up to
# a power of two: 16 u.  By analysis three roundings of relative size u leave at most (1 + 2 a) u (|e| + |p'|), 2.8 u at a = 0.9
# and under 4 u for any a < 1: a figure beyond 4 u on the device would mean that the formula is not the one specified.
E_BOUND = 16.0


@functools.lru_cache(maxsize=None)
def adam_ema_data(n):
    """(p, g, m, v, e, dead, pad) of n + PAD floats each, on the CPU: the recipe of tests/test_train_tail.py::_adam_data (|g| log-
    uniform in [1e-6, 10] with random sign and a share of exact zeros, m ~ 0.1 N, v ~ 0.1 U, `dead` elements with g = m = v = 0)
    plus e ~ N(0, 1) independent of p, and `pad`, a part of the dead elements where p = e = 0 as well: the flat buffers' padding."""
    gen = torch.Generator().manual_seed(n)
    N = n + PAD
    p = torch.randn(N, generator=gen)
    g = 10.0 ** (7.0 * torch.rand(N, generator=gen) - 6.0) * (2.0 * torch.randint(0, 2, (N,), generator=gen) - 1.0)
    g[torch.rand(N, generator=gen) < 0.15] = 0.0
    m = 0.1 * torch.randn(N, generator=gen)
    v = 0.1 * torch.rand(N, generator=gen)
    dead = torch.rand(N, generator=gen) < 0.1
    if n >= 5:
        dead[1:3] = True                       # inside [offset, offset + n) for both offsets
        dead[3] = False
    for t in (g, m, v):
        t[dead] = 0.0
    e = torch.randn(N, generator=gen)
    pad = dead & (torch.rand(N, generator=gen) < 0.5)
    if n >= 5:
        pad[2] = True
    p[pad] = 0.0
    e[pad] = 0.0
    return p, g, m, v, e, dead, pad


def ema_weight(ema_rate, ema_warm, k):
    """The weight as the kernel forms it: the fp32 ema_rate the ABI receives, the warm-up in fp64, one rounding to fp32."""
    rate = float(np.float32(ema_rate))
    return float(np.float32(max(rate, 9.0 / (10.0 + k)) if ema_warm else rate))


def ema_ref(e, p_new, a):
    """fp64: e + a (p' - e)."""
    e, p_new = e.double(), p_new.double()
    return e + a * (p_new - e)


def adam_np32(p, g, m, v, state=STATE, lr=LR, b1=B1, b2=B2, eps=EPS):
    """The parameters after the update, by the kernel's sequence of fp32 operations in numpy (csrc/train_ops.hip: adam_update) for a
    state with an imposed rate.  Only the CPU derivation of E_BOUND uses it; on the GPU p' is the device's own."""
    f = np.float32
    p, g, m, v = (t.numpy().astype(f) for t in (p, g, m, v))
    t, rate = float(f(state[0])), f(state[3])
    b1, b2, eps = f(b1), f(b2), f(eps)
    step_size = f(float(rate) / (1.0 - float(b1) ** t))
    inv_sqrt_bc2 = f(1.0 / np.sqrt(1.0 - float(b2) ** t))
    m1 = b1 * m + (f(1.0) - b1) * g
    v1 = b2 * v + (f(1.0) - b2) * g * g
    denom = np.sqrt(v1) * inv_sqrt_bc2 + eps
    return torch.from_numpy(p - step_size * (m1 / denom))


def ema_np32(e, p_new, a):
    """e + a (p' - e) as the kernel evaluates it: three fp32 operations, no contraction."""
    e, p_new, a = e.numpy().astype(np.float32), p_new.numpy().astype(np.float32), np.float32(a)
    return torch.from_numpy(e + a * (p_new - e))


def units(got, want, scale):
    """max over elements of |got - want| / (u * scale); where the scale is 0 the values must agree exactly."""
    got, want, scale = got.detach().cpu().double().reshape(-1), want.detach().double().reshape(-1), scale.detach().double().reshape(-1)
    err = (got - want).abs()
    zero = scale == 0
    assert bool((err[zero] == 0).all()), "difference where the operands are all zero"
    if bool(zero.all()):
        return 0.0
    return float((err[~zero] / (U * scale[~zero])).max())
