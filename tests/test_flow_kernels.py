"""The kernels of csrc/flows.hip one by one, through the C ABI (glow_tts_train._hip.call), against plain fp64 torch on the CPU:
mask_len, actnorm_fwd (forward, reverse) / _bwd / _stats, invconv_prepare / _prepare_multi, invconv_fwd / _bwd (n_split 2, 4, 8:
register kernels; 6, 32: run-time-N kernels), actnorm_invconv_fwd / _bwd, coupling_fwd (forward, reverse) / _bwd and
coupling_actnorm_invconv_fwd / _bwd, all fp32 (io = 0).  The golden tests reach these kernels through layers.* and autograd at
rtol 2e-4 on sums of 1e4 .. 1e6 terms, where a dropped element, a slab counted twice or a log-det term added once too often is
invisible; coupling_actnorm_invconv_* is otherwise only the "want" side of the flow_boundary tests.  The GPU tests are marked
`gpu`; the tests at the end of the module are not: they check the table below on the CPU.

References: oracle.glow_oracle.actnorm, invconv_matrix_apply, the coupling formulas of oracle.glow_oracle.coupling (lines 231-242)
and their compositions, in fp64; gradients by autograd in fp64 (log det W through torch.logdet).  The raw ABI takes w_inv, logdet_w
and x_len as ARGUMENTS: they come from fp64, rounded once to fp32, so invconv_prepare is tested on its own.  W is never symmetric
and never orthogonal (W, W^-1 and W^-T differ).

Every launch (_Dev): each input is a copy inside a guarded buffer and must be bit-identical afterwards; each output lives between
GUARD sentinels that must survive, and is pre-filled with GUARD (written outputs) or with its starting value (accumulated ones:
dlogs, dbias, dW, the stats sums and the coupling's log-det, which include/glowtts_hip.h documents as "atomically ADDED to: the
caller zeroes them or passes a running sum" — every such output is tested from 0 at every shape and from a running sum of
small integers at (3, 8, 36); the coupling's log-dets from both at every shape).  Inputs beyond an utterance's length hold random finite values;
every masked output there must be exactly 0 (the coupling's pass-through half z0 = x0 / dx0 = dz0 is a copy, as in the oracle);
one row has length 0 once B >= 2: exactly zero outputs, logdet[b] == 0 (its starting value), no contribution to any sum.

Two kinds of input.
  1. Counting inputs: logs = 0 (expf gives exactly 1); x, dz, bias, m, dlogdet small integers in [-2, 2]; raw logs' = 0 ("count":
     everything is checked) or a small integer ("countld": only the log-det sums are checked); W an integer unimodular matrix
     (unit upper bidiagonal times a permutation: W^-1 is an integer matrix with entries in {-1, 0, 1}), handed over with its
     integer inverse; logdet_w is handed over as the integer 3 (an independent argument of the ABI; with 0 every log-det would be
     0 whatever the kernel multiplies it with).  Every partial sum is an integer below 2**24 (asserted per case from the sum of
     absolute terms, before the launch), hence exact in fp32 in any order and under any contraction: ALL outputs are asserted
     EQUAL to the fp64 result.  sigmoid_scale = 0 only (log(1e-6 + sigmoid(2)) is no integer).
  2. Random inputs: logs ~ 0.3 N, bias ~ 0.5 N, x, dz ~ N, W = QR factor + 0.1 N with det > 0 and cond <= 100, raw logs' ~ 0.3 N,
     m ~ 0.5 N, dlogdet ~ N.  Bounds (u = 2**-24):
       * reductions (dlogs, dbias, dW, log-dets, stats): |got - want| <= 1e-5 * sum|term_i|, the project's figure for "block sum +
         one float atomic per workgroup" (tests/test_grad_accum.py::test_clip_grad_value_scaled_vs_torch, tests/test_train_tail.py);
       * element-wise outputs: per element, in units of u times the magnitude of the operands of the output's last operation
         (e.g. sum_o |W[o][k]| |dz[o]| for InvConv's dx); the bound is 4 x what plain fp32 torch on the CPU shows against fp64 on
         the same inputs (the reference alone, worst over TABLE_SHAPES), rounded up to a power of two:
             output                            scale                                                   fp32 CPU   bound
             actnorm z                         (|bias| + |e x|) mask                                   2.46 u     16 u
             actnorm reverse                   (|x| + |bias|) e^-logs mask                             2.78 u     16 u
             actnorm dx                        |dx|                                                    1.89 u      8 u
             invconv z                         sum_k |W[o][k]| |x_k| mask                              3.00 u     16 u
             invconv dx                        sum_o |W[o][k]| |dz_o| mask                             3.27 u     16 u
             actnorm_invconv z                 sum_k |W[o][k]| (|bias_k| + |e_k x_k|) mask             3.44 u     16 u
             actnorm_invconv dx, S             e_k sum_o |W[o][k]| |dz_o| mask                         3.90 u     16 u
             coupling z1                       (|m| + |e^logs' x1|) mask                               3.33 u     16 u
             coupling reverse                  (|x1| + |m|) e^-logs' mask                              4.22 u     32 u
             coupling dx1                      |dx1|                                                   2.74 u     16 u
             coupling dlogs', sig = 0          (|dz1 e^logs' x1| + |dlogdet|) mask                     2.83 u     16 u
             coupling dlogs', sig = 1          the same times |dlogs'/draw|                            27.0 u    128 u
             coupling_ai y                     sum_k |W[o][k]| (|bias_k| + e_k Z_k) mask, Z as z1      3.66 u     16 u
             coupling_ai dy_prev, 1st half     S                                                       3.90 u     16 u
             coupling_ai dy_prev, 2nd half     S e^logs'                                               4.98 u     32 u
             coupling_ai dout_prev (dm)        S                                                       3.90 u     16 u
             coupling_ai dout_prev (dlogs'), 0 S e^logs' |y1| + |dlogdet| mask                         4.74 u     32 u
             coupling_ai dout_prev (dlogs'), 1 the same times |dlogs'/draw|                            28.5 u    128 u
         (dlogs' has a bound for each sigmoid_scale: with 1, dlogs'/draw = s (1 - s) / (1e-6 + s) loses digits in 1 - s; with 0
         there is no such factor.  The worst figures come from the shape with the most elements, (2, 400, 1001).)  fp32 torch's
         reductions are at most 8.8e-7 of sum|term| on these inputs; InvConv's log-det and dW, which in the fp32 reference go
         through fp32 torch.logdet and its gradient, 6.2e-6: no kernel here computes those (w_inv and logdet_w are arguments).
         The CPU test prints the two figures apart.
         copies (z0, dx0, the coupling's dm = dz1 mask): 0 u.  The CPU tests at the end of the module recompute the fp32 column
         and assert fig <= bound <= 16 fig, so a bound cannot be widened afterwards.  Each GPU test prints its figures (-s);
       * invconv_prepare works in fp64 internally, so its bound is derived: |w_inv - inv64| <= 2**-24 |inv64| + 1e-9 max|inv64|,
         |logdet - logdet64| <= 2**-24 |logdet64| + 1e-9, for cond <= 100 (asserted for every matrix) and n <= 32.

Shapes (B, C, T): the smallest that take each branch of the launchers at the end of flows.hip; each says which, in prose and as
the fields of the plan the library hands back (glowtts_flow_plan_for, csrc/flow_plan.hpp): section 9 asks it on the CPU, for every
row and every shape, and compares it over a sweep with _parent_rules, the launch rules as the launchers had them inline.
"""
import functools
import math
import re
import types

import pytest
import torch

gpu = pytest.mark.gpu

U = 2.0 ** -24
GUARD = -1234.5          # sentinel in front of and behind every raw-ABI output
PAD = 8                  # floats of guard on each side (32 bytes: the payload stays 16-byte aligned)

# element-wise bounds in u (the table of the module docstring)
BOUNDS = {"an_z": 16, "an_rev": 16, "an_dx": 8, "ic_z": 16, "ic_dx": 16, "ai_z": 16, "ai_dx": 16,
          "cp_z1": 16, "cp_rev": 32, "cp_dx1": 16, "cp_dl0": 16, "cp_dl1": 128,
          "ca_y": 16, "ca_dy": 32, "ca_dm": 16, "ca_dl0": 32, "ca_dl1": 128, "copy": 0}


@pytest.fixture(scope="module")
def G():
    from glow_tts_train import _hip

    _hip.load()
    return types.SimpleNamespace(hip=_hip)


def _O():
    from oracle import glow_oracle

    return glow_oracle


def _units(got, want, scale):
    """max over elements of |got - want| / (u * scale); where the scale is 0 the values must agree exactly."""
    got, want, scale = got.detach().cpu().double().reshape(-1), want.detach().double().reshape(-1), scale.detach().double().reshape(-1)
    err = (got - want).abs()
    zero = scale == 0
    assert bool((err[zero] == 0).all()), "difference where the operands are all zero"
    if bool(zero.all()):
        return 0.0
    return float((err[~zero] / (U * scale[~zero])).max())


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _ragged(gen, B, T, empty_row=True):
    """Lengths in [1, T] with row 0 full and, from two rows on, one row of length 0."""
    lengths = torch.randint(1, T + 1, (B,), generator=gen)
    lengths[0] = T
    if empty_row and B >= 2:
        lengths[B // 2] = 0
    return lengths


def _mask(lengths, T):
    return (torch.arange(T)[None] < lengths[:, None]).float()


# =============================================================================================== inputs
def _cond(w64):
    s = torch.linalg.svdvals(w64)
    return float(s[0] / s[-1])


def _random_w(n, seed, want_det=1):
    """QR factor + 0.1 N in fp64, rounded once to fp32; det of the wanted sign, cond <= 100."""
    for s in range(seed, seed + 200):
        gen = torch.Generator().manual_seed(s)
        w = torch.linalg.qr(torch.randn(n, n, generator=gen, dtype=torch.float64))[0] + 0.1 * torch.randn(n, n, generator=gen, dtype=torch.float64)
        if float(torch.det(w)) * want_det < 0:
            w[:, -1] = -w[:, -1]
        w = w.float()
        if _cond(w.double()) <= 100:
            return w
    raise AssertionError("no well-conditioned matrix found")


def _count_w(n, seed):
    """Integer unimodular W = (I + superdiagonal in {-1, 0, 1}) x permutation, with W, W^-1, W^-T pairwise different."""
    for s in range(seed, seed + 200):
        gen = torch.Generator().manual_seed(s)
        u = torch.eye(n, dtype=torch.float64)
        sup = torch.randint(-1, 2, (n - 1,), generator=gen).double()
        sup[0] = 1.0
        u += torch.diag(sup, 1)
        w = u[:, torch.randperm(n, generator=gen)]
        inv = torch.linalg.inv(w).round()
        if not torch.equal(w @ inv, torch.eye(n, dtype=torch.float64)) or float(inv.abs().max()) > 1:
            continue
        if torch.equal(w, w.T) or torch.equal(w, inv) or torch.equal(w, inv.T) or torch.equal(inv, inv.T):
            continue
        return w.float(), inv.float()
    raise AssertionError("no integer matrix found")


@functools.lru_cache(maxsize=8)
def _inputs(kind, B, C, T, n, seed=0):
    """Everything any kernel of the module reads, fp32 on the CPU.  x doubles as y_prev, `out` = [m ; raw logs']."""
    gen = torch.Generator().manual_seed(1000003 * seed + 7919 * B + 104729 * C + T + n + len(kind))
    I = types.SimpleNamespace(kind=kind, B=B, C=C, T=T, n=n)
    I.lengths = _ragged(gen, B, T)
    I.mask = _mask(I.lengths, T)
    I.x_len = I.lengths.float()
    if kind.startswith("count"):
        ri = lambda *shape: torch.randint(-2, 3, shape, generator=gen).float()
        I.x, I.dz, I.bias, I.dld = ri(B, C, T), ri(B, C, T), ri(C), ri(B)
        I.logs = torch.zeros(C)
        I.out = ri(B, C, T)
        if kind == "count":
            I.out[:, C // 2:] = 0.0
        I.w, I.w_inv = _count_w(n, seed + n) if n else (None, None)
        I.logdet_w = torch.tensor([3.0])
    else:
        I.x, I.dz, I.dld = torch.randn(B, C, T, generator=gen), torch.randn(B, C, T, generator=gen), torch.randn(B, generator=gen)
        I.logs, I.bias = 0.3 * torch.randn(C, generator=gen), 0.5 * torch.randn(C, generator=gen)
        I.out = torch.cat([0.5 * torch.randn(B, C // 2, T, generator=gen), 0.3 * torch.randn(B, C - C // 2, T, generator=gen)], 1)
        if n:
            I.w = _random_w(n, seed + 31 * n)
            w64 = I.w.double()
            assert not torch.allclose(w64, w64.T, atol=1e-2) and not torch.allclose(w64 @ w64.T, torch.eye(n, dtype=torch.float64), atol=1e-2)
            I.w_inv, I.logdet_w = torch.linalg.inv(w64).float(), torch.logdet(w64).float().reshape(1)
    if n:
        assert _cond(I.w.double()) <= 100
    return I


# =============================================================================================== the fp64 (or fp32) reference
def _start_like(start, shape):
    """The starting value of an accumulated output of `shape`: the entries of `start`, repeated as often as needed."""
    numel = int(math.prod(shape))
    return start.reshape(-1)[torch.arange(numel) % start.numel()].reshape(shape)


def _rows(x, n):
    """(B, C, T) -> (B, G, n, T): row k of group g is channel (k // (n/2)) (C/2) + g (n/2) + k % (n/2)  (layers.py:247-252)."""
    B, C, T = x.shape
    return x.reshape(B, 2, C // n, n // 2, T).permute(0, 2, 1, 3, 4).reshape(B, C // n, n, T)


def _pair_sum(a, b, n):
    """[o][k] -> sum over (b, g, t) of a[row o] b[row k]."""
    return torch.einsum("bgot,bgkt->ok", _rows(a, n), _rows(b, n))


class _Res(dict):
    """name -> (kind, value, scale): kind 'e:<bound key>' element-wise (scale per element, masked outputs flagged by 'm' in
    the flags), 's' reduction (scale = sum |term|)."""

    def elem(self, name, key, value, scale, masked=True):
        self[name] = ("e", key, value.detach(), scale.detach(), masked)

    def red(self, name, value, abs_terms, start=None):
        """`start`: what an accumulated output held before the call; the kernel has to add to it."""
        if start is not None:
            start = _start_like(start, value.shape)
            value, abs_terms = start.to(value.dtype) + value, start.to(value.dtype).abs() + abs_terms
        self[name] = ("s", None, value.detach(), abs_terms.detach(), start)


def _ref(op, I, dt, sig=0, dld=True, rev=False, start=None):
    """The operation `op` on the inputs I in dtype dt with plain torch on the CPU; gradients by autograd."""
    O = _O()
    n, B, C, T = I.n, I.B, I.C, I.T
    c = lambda t: None if t is None else t.to(dt)
    x, dz, mask, x_len = c(I.x), c(I.dz), c(I.mask)[:, None], c(I.x_len)
    logs, bias, out = c(I.logs), c(I.bias), c(I.out)
    dl = c(I.dld) if dld else torch.zeros(B, dtype=dt)
    G_ = C // n if n else 0
    R = _Res()
    mix = lambda a, w: O.invconv_matrix_apply(a, w, n)
    dterm = (dl * x_len).abs().sum()

    def logdet_of(w):
        """log det W as a function of W: torch.logdet for the random matrices; for the counting ones the value handed to the
        kernel (an independent argument) with the gradient W^-T taken from the exact integer inverse."""
        if I.kind == "random":
            return torch.logdet(w)
        return c(I.logdet_w)[0] + ((w - w.detach()) * c(I.w_inv).T).sum()

    def cpl_logs(raw):
        return torch.log(1e-6 + torch.sigmoid(raw + 2)) if sig else raw

    def chain(raw):
        s = torch.sigmoid(raw + 2)
        return s * (1 - s) / (1e-6 + s) if sig else torch.ones_like(raw)

    h = C // 2
    if op == "mask_len":
        R.red("x_len", mask.sum((1, 2)), mask.sum((1, 2)))
    elif op == "actnorm_fwd":
        l3, b3 = logs.view(1, C, 1), bias.view(1, C, 1)
        z, ld = O.actnorm(x, mask, l3, b3, reverse=rev)
        if rev:
            R.elem("z", "an_rev", z, (x.abs() + b3.abs()) * torch.exp(-l3) * mask)
        else:
            R.elem("z", "an_z", z, (b3.abs() + (torch.exp(l3) * x).abs()) * mask)
            R.red("logdet", ld, logs.abs().sum() * x_len)
    elif op == "actnorm_stats":
        R.red("sum_x", (x * mask).sum((0, 2)), (x.abs() * mask).sum((0, 2)), start)
        R.red("sum_x2", (x * x * mask).sum((0, 2)), (x * x * mask).sum((0, 2)), start)
    elif op == "actnorm_bwd":
        xr, lr, br = x.clone().requires_grad_(True), logs.clone().requires_grad_(True), bias.clone().requires_grad_(True)
        z, ld = O.actnorm(xr, mask, lr.view(1, C, 1), br.view(1, C, 1))
        ((z * dz).sum() + (ld * dl).sum()).backward()
        e3 = torch.exp(logs).view(1, C, 1)
        R.elem("dx", "an_dx", xr.grad, xr.grad.abs())
        R.red("dlogs", lr.grad, (dz.abs() * e3 * x.abs() * mask).sum((0, 2)) + dterm, start)
        R.red("dbias", br.grad, (dz.abs() * mask).sum((0, 2)), start)
    elif op == "invconv_fwd":
        w = c(I.w)
        R.elem("z", "ic_z", mix(x, w) * mask, mix(x.abs(), w.abs()) * mask)
        ld = logdet_of(w) * G_ * x_len
        R.red("logdet", ld, ld.abs())
    elif op == "invconv_bwd":
        xr, wr = x.clone().requires_grad_(True), c(I.w).clone().requires_grad_(True)
        z = mix(xr, wr) * mask
        ((z * dz).sum() + (logdet_of(wr) * G_ * x_len * dl).sum()).backward()
        gz = dz * mask
        R.elem("dx", "ic_dx", xr.grad, mix(gz.abs(), c(I.w).abs().T.contiguous()))
        R.red("dw", wr.grad, _pair_sum(gz.abs(), x.abs(), n) + c(I.w_inv).abs().T * G_ * dterm, start)
    elif op in ("actnorm_invconv_fwd", "actnorm_invconv_bwd", "coupling_ai_fwd", "coupling_ai_bwd"):
        fused_cpl = op.startswith("coupling_ai")
        leaves = [t.clone().requires_grad_(True) for t in (x, out, logs, bias, c(I.w))]
        xr, outr, lr, br, wr = leaves
        l3, b3 = lr.view(1, C, 1), br.view(1, C, 1)
        if fused_cpl:                                        # z = the affine apply of the previous block on (y_prev, out_prev)
            lp = cpl_logs(outr[:, h:])
            zin = torch.cat([xr[:, :h], (outr[:, :h] + torch.exp(lp) * xr[:, h:]) * mask], 1)
            ld_prev = (lp * mask).sum((1, 2))
            el = torch.exp(lp).detach()
            zabs = torch.cat([x[:, :h].abs(), (out[:, :h].abs() + (el * x[:, h:]).abs()) * mask], 1)
        else:
            zin, ld_prev, zabs = xr, torch.zeros(B, dtype=dt), x.abs()
        y, _ = O.actnorm(zin, mask, l3, b3)
        z = mix(y, wr) * mask
        ld = (lr.sum() + logdet_of(wr) * G_) * x_len
        e3 = torch.exp(logs).view(1, C, 1)
        wabs = c(I.w).abs()
        if op.endswith("fwd"):
            R.elem("y" if fused_cpl else "z", "ca_y" if fused_cpl else "ai_z", z, mix((bias.view(1, C, 1).abs() + e3 * zabs) * mask, wabs) * mask)
            R.red("logdet", ld, (logs.abs().sum() + logdet_of(c(I.w)).abs() * G_) * x_len)
            if fused_cpl:
                R.red("logdet_prev", ld_prev, (lp.detach().abs() * mask).sum((1, 2)), start)
            return R
        ((z * dz).sum() + ((ld + ld_prev) * dl).sum()).backward()
        gz = dz * mask
        dy = mix(gz, c(I.w).T.contiguous()) * mask           # gradient of the ActNorm output
        S = mix(gz.abs(), wabs.T.contiguous()) * mask * e3   # magnitude of the operands of the gradient of z
        zv, yv = zin.detach(), y.detach()
        R.red("dlogs", lr.grad, (dy.abs() * e3 * zv.abs()).sum((0, 2)) + dterm, start)
        R.red("dbias", br.grad, dy.abs().sum((0, 2)), start)
        R.red("dw", wr.grad, _pair_sum(gz.abs(), yv.abs(), n) + c(I.w_inv).abs().T * G_ * dterm, start)
        if not fused_cpl:
            R.elem("dx", "ai_dx", xr.grad, S)
        else:
            ch = chain(out[:, h:])
            R.elem("dy0", "ai_dx", xr.grad[:, :h], S[:, :h])
            R.elem("dy1", "ca_dy", xr.grad[:, h:], S[:, h:] * el)
            R.elem("dm", "ca_dm", outr.grad[:, :h], S[:, h:])
            R.elem("dl", f"ca_dl{int(bool(sig))}", outr.grad[:, h:], (S[:, h:] * el * x[:, h:].abs() + dl.abs().view(B, 1, 1) * mask) * ch)
    elif op == "coupling_fwd":
        lp = cpl_logs(out[:, h:])
        m, x0, x1 = out[:, :h], x[:, :h], x[:, h:]
        R.elem("z0", "copy", x0, x0.abs(), masked=False)
        if rev:
            R.elem("z1", "cp_rev", (x1 - m) * torch.exp(-lp) * mask, (x1.abs() + m.abs()) * torch.exp(-lp) * mask)
        else:
            R.elem("z1", "cp_z1", (m + torch.exp(lp) * x1) * mask, (m.abs() + (torch.exp(lp) * x1).abs()) * mask)
            R.red("logdet", (lp * mask).sum((1, 2)), (lp.abs() * mask).sum((1, 2)), start)
    elif op == "coupling_bwd":
        xr, outr = x.clone().requires_grad_(True), out.clone().requires_grad_(True)
        lp = cpl_logs(outr[:, h:])
        z = torch.cat([xr[:, :h], (outr[:, :h] + torch.exp(lp) * xr[:, h:]) * mask], 1)
        ((z * dz).sum() + ((lp * mask).sum((1, 2)) * dl).sum()).backward()
        el = torch.exp(lp).detach()
        R.elem("dx0", "copy", xr.grad[:, :h], xr.grad[:, :h].abs(), masked=False)
        R.elem("dx1", "cp_dx1", xr.grad[:, h:], xr.grad[:, h:].abs())
        R.elem("dm", "copy", outr.grad[:, :h], outr.grad[:, :h].abs())
        R.elem("dl", f"cp_dl{int(bool(sig))}", outr.grad[:, h:], ((dz[:, h:] * el * x[:, h:]).abs() + dl.abs().view(B, 1, 1)) * mask * chain(out[:, h:]))
    else:
        raise KeyError(op)
    return R


# =============================================================================================== the launches
class _Dev:
    """The buffers of one raw-ABI call: inputs are copies inside guarded buffers (bit-identical afterwards), outputs live between
    GUARD sentinels.  `mis` names the one tensor that starts one float off a 16-byte boundary."""

    def __init__(self, mis=None):
        self.mis, self.ins, self.outs, self.seen = mis, [], [], set()

    def _place(self, name, numel):
        off = 1 if name == self.mis else 0
        self.seen.add(name)
        buf = torch.full((numel + 2 * PAD,), GUARD, device="cuda")
        view = buf[PAD + off: PAD + off + numel]
        assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4 * off
        return buf, view, off

    def inp(self, name, t):
        if t is None:
            return None
        buf, view, off = self._place(name, t.numel())
        view.copy_(t.reshape(-1))
        self.ins.append((name, t, buf, off))
        return view.data_ptr()

    def out(self, name, shape, init=None):
        numel = int(math.prod(shape))
        buf, view, off = self._place(name, numel)
        if init is not None:
            view.copy_(_start_like(init, (numel,)).float() if torch.is_tensor(init) else torch.full((numel,), float(init)))
        self.outs.append((name, shape, buf, off, numel))
        return view.data_ptr()

    def finish(self):
        torch.cuda.synchronize()
        assert self.mis is None or self.mis in self.seen, self.mis
        for name, t, buf, off in self.ins:
            b = buf.cpu()
            lo, hi = PAD + off, PAD + off + t.numel()
            assert _bits_equal(b[lo:hi], t.reshape(-1)), f"input {name} changed"
            assert bool((b[:lo] == GUARD).all()) and bool((b[hi:] == GUARD).all()), f"written around input {name}"
        res = {}
        for name, shape, buf, off, numel in self.outs:
            b = buf.cpu()
            lo, hi = PAD + off, PAD + off + numel
            assert bool((b[:lo] == GUARD).all()) and bool((b[hi:] == GUARD).all()), f"guard of output {name} overwritten"
            res[name] = b[lo:hi].reshape(shape).clone()
        return res


# tensors of each entry point that the vector kernels read or write 16 bytes at a time (the arguments of can_vec4)
VEC_TENSORS = {"actnorm_fwd": ("x", "mask", "z"), "actnorm_bwd": ("x", "mask", "dz", "dx"), "actnorm_stats": ("x", "mask"),
               "invconv_fwd": ("x", "mask", "z"), "invconv_bwd": ("x", "mask", "dz", "dx"),
               "actnorm_invconv_fwd": ("x", "mask", "z"), "actnorm_invconv_bwd": ("x", "mask", "dz", "dx"),
               "coupling_fwd": ("x", "out", "mask", "z"), "coupling_bwd": ("x", "out", "mask", "dz", "dx", "dout"),
               "coupling_ai_fwd": ("x", "out", "mask", "y"), "coupling_ai_bwd": ("x", "out", "mask", "dz", "dx", "dout")}


def _launch(G, op, I, sig=0, dld=True, rev=False, start=None, mis=None, D=None):
    """One call of the entry point behind `op`; returns name -> CPU tensor, named as in _ref."""
    D = D or _Dev(mis)
    B, C, T, n, h = I.B, I.C, I.T, I.n, I.C // 2
    call = G.hip.call
    zero = 0.0 if start is None else start
    dl = lambda: D.inp("dlogdet", I.dld) if dld else None
    xl = lambda: D.inp("x_len", I.x_len)
    if op == "mask_len":
        call("glowtts_mask_len", D.inp("mask", I.mask), D.out("x_len", (B,)), B, T)
        return D.finish()
    if op == "actnorm_fwd":
        call("glowtts_actnorm_fwd", D.inp("x", I.x), D.inp("mask", I.mask), D.inp("logs", I.logs), D.inp("bias", I.bias), xl(),
             D.out("z", (B, C, T)), None if rev else D.out("logdet", (B,)), B, C, T, int(rev))
        return D.finish()
    if op == "actnorm_stats":
        call("glowtts_actnorm_stats", D.inp("x", I.x), D.inp("mask", I.mask), D.out("sum_x", (C,), zero), D.out("sum_x2", (C,), zero), B, C, T)
        return D.finish()
    if op == "actnorm_bwd":
        call("glowtts_actnorm_bwd", D.inp("x", I.x), D.inp("mask", I.mask), D.inp("logs", I.logs), D.inp("dz", I.dz), dl(), xl(),
             D.out("dx", (B, C, T)), D.out("dlogs", (C,), zero), D.out("dbias", (C,), zero), B, C, T)
        return D.finish()
    if op == "invconv_fwd":
        call("glowtts_invconv_fwd", D.inp("x", I.x), D.inp("mask", I.mask), D.inp("w", I.w), D.inp("logdet_w", I.logdet_w), xl(),
             D.out("z", (B, C, T)), D.out("logdet", (B,)), B, C, T, n)
        return D.finish()
    if op == "invconv_bwd":
        call("glowtts_invconv_bwd", D.inp("x", I.x), D.inp("mask", I.mask), D.inp("w", I.w), D.inp("w_inv", I.w_inv), D.inp("dz", I.dz),
             dl(), xl(), D.out("dx", (B, C, T)), D.out("dw", (n, n), zero), B, C, T, n)
        return D.finish()
    if op == "actnorm_invconv_fwd":
        call("glowtts_actnorm_invconv_fwd", D.inp("x", I.x), D.inp("mask", I.mask), D.inp("logs", I.logs), D.inp("bias", I.bias),
             D.inp("w", I.w), D.inp("logdet_w", I.logdet_w), xl(), D.out("z", (B, C, T)), D.out("logdet", (B,)), B, C, T, n)
        return D.finish()
    if op == "actnorm_invconv_bwd":
        call("glowtts_actnorm_invconv_bwd", D.inp("x", I.x), D.inp("mask", I.mask), D.inp("logs", I.logs), D.inp("bias", I.bias),
             D.inp("w", I.w), D.inp("w_inv", I.w_inv), D.inp("dz", I.dz), dl(), xl(), D.out("dx", (B, C, T)),
             D.out("dlogs", (C,), zero), D.out("dbias", (C,), zero), D.out("dw", (n, n), zero), B, C, T, n)
        return D.finish()
    if op == "coupling_fwd":
        call("glowtts_coupling_fwd", D.inp("x", I.x), D.inp("out", I.out), D.inp("mask", I.mask), D.out("z", (B, C, T)),
             None if rev else D.out("logdet", (B,), zero), B, C, T, sig, int(rev))
        r = D.finish()
        r["z0"], r["z1"] = r["z"][:, :h], r.pop("z")[:, h:]
        return r
    if op == "coupling_bwd":
        call("glowtts_coupling_bwd", D.inp("x", I.x), D.inp("out", I.out), D.inp("mask", I.mask), D.inp("dz", I.dz), dl(),
             D.out("dx", (B, C, T)), D.out("dout", (B, C, T)), B, C, T, sig)
        r = D.finish()
        r["dx0"], r["dx1"], r["dm"], r["dl"] = r["dx"][:, :h], r.pop("dx")[:, h:], r["dout"][:, :h], r.pop("dout")[:, h:]
        return r
    if op == "coupling_ai_fwd":
        call("glowtts_coupling_actnorm_invconv_fwd", D.inp("x", I.x), D.inp("out", I.out), D.inp("mask", I.mask), D.inp("logs", I.logs),
             D.inp("bias", I.bias), D.inp("w", I.w), D.inp("logdet_w", I.logdet_w), xl(), D.out("y", (B, C, T)),
             D.out("logdet_prev", (B,), zero), D.out("logdet", (B,)), B, C, T, n, sig)
        return D.finish()
    if op == "coupling_ai_bwd":
        call("glowtts_coupling_actnorm_invconv_bwd", D.inp("x", I.x), D.inp("out", I.out), D.inp("mask", I.mask), D.inp("logs", I.logs),
             D.inp("bias", I.bias), D.inp("w", I.w), D.inp("w_inv", I.w_inv), D.inp("dz", I.dz), dl(), xl(),
             D.out("dx", (B, C, T)), D.out("dout", (B, C, T)), D.out("dlogs", (C,), zero), D.out("dbias", (C,), zero),
             D.out("dw", (n, n), zero), B, C, T, n, sig)
        r = D.finish()
        r["dy0"], r["dy1"], r["dm"], r["dl"] = r["dx"][:, :h], r.pop("dx")[:, h:], r["dout"][:, :h], r.pop("dout")[:, h:]
        return r
    raise KeyError(op)


PER_UTTERANCE = ("x_len", "logdet", "logdet_prev")


def _compare(op, I, got, want, what, only=None):
    """Counting inputs: every output EQUAL to the fp64 result.  Random inputs: the bounds of the module docstring.
    Both: exactly 0 behind every utterance's end, and the row of length 0 leaves its log-det at the starting value."""
    figs = []
    behind = (I.mask == 0)[:, None]
    empty = I.lengths == 0
    assert set(got) == set(want), (sorted(got), sorted(want))
    for name, (kind, key, value, scale, extra) in want.items():
        g = got[name]
        assert g.shape == value.shape, (name, g.shape, value.shape)
        assert bool(torch.isfinite(g).all()), f"{what} {name}: non-finite output"
        if only is not None and name not in only:
            continue
        if kind == "e" and extra:
            assert bool((g[behind.expand_as(g)] == 0).all()), f"{what} {name}: not exactly 0 behind an utterance's end"
        if name in PER_UTTERANCE and bool(empty.any()):
            st = torch.zeros(I.B) if extra is None else extra.float()
            assert torch.equal(g[empty], st[empty]), f"{what} {name}: the empty row contributes"
        if I.kind.startswith("count"):
            assert torch.equal(g.double(), value.double()), f"{what} {name}: differs from integer arithmetic by up to {float((g.double() - value).abs().max())}"
            figs.append(f"{name} ==")
        elif kind == "e":
            fig, bound = _units(g, value, scale), BOUNDS[key]
            figs.append(f"{name} {fig:.2f} u (bound {bound})")
            assert fig <= bound, f"{what} {name}: {fig:.2f} u > {bound} u"
        else:
            err, sc = (g.double() - value).abs(), scale.double()
            assert bool((err[sc == 0] == 0).all()), f"{what} {name}: difference where every term is 0"
            fig = float((err[sc > 0] / sc[sc > 0]).max()) if bool((sc > 0).any()) else 0.0
            figs.append(f"{name} {fig:.1e} of sum|term| (bound 1e-5)")
            assert fig <= 1e-5, f"{what} {name}: {fig:.2e} of sum|term| > 1e-5"
    print(f"{what}: " + "; ".join(figs))


def _assert_exact_range(want, what):
    """Counting inputs: the sum of absolute terms bounds every partial sum in any order; below 2**24 all of them are exact."""
    for name, (kind, _key, value, scale, _extra) in want.items():
        top = float(scale.abs().max()) if scale.numel() else 0.0
        assert top < 2 ** 24, (what, name, top)
        assert bool((value == value.round()).all()), (what, name)


def _run(G, op, shape, n=0, sigs=(0,), dlds=(True,), revs=(False,), kinds=("count", "random"), misalign=False, running_sum=False):
    """Every variant of `op` at one shape.  running_sum: the accumulated outputs also start from small integers instead of 0."""
    B, C, T = shape
    per_b = op in ("coupling_fwd", "coupling_ai_fwd")
    run_sum = torch.randint(1, 4, (B if per_b else C,), generator=torch.Generator().manual_seed(B + C)).float()
    for kind in kinds:
        I = _inputs(kind, B, C, T, n)
        for sig, dld, rev, st in [(s, d, r, t) for s in sigs for d in dlds for r in revs for t in ((None, run_sum) if running_sum else (None,))]:
            if sig and kind != "random":
                continue                                     # log(1e-6 + sigmoid(2)) is no integer: sigmoid_scale = 1 has no counting form
            if rev and (kind == "countld" or st is not None):
                continue                                     # the reverse has no log-det
            want = _ref(op, I, torch.float64, sig=sig, dld=dld, rev=rev, start=st)
            only = ("logdet", "logdet_prev") if kind == "countld" else None
            if kind.startswith("count"):
                _assert_exact_range({k: v for k, v in want.items() if only is None or k in only}, (op, shape, n))
            for mis in [None] + (list(VEC_TENSORS[op]) if misalign else []):
                what = f"{op} {kind} {shape} n={n} sig={sig} dlogdet={int(dld)} rev={int(rev)} start={'0' if st is None else 'sum'}" \
                       + (f" misaligned={mis}" if mis else "")
                got = _launch(G, op, I, sig=sig, dld=dld, rev=rev, start=st, mis=mis)
                _compare(op, I, got, want, what, only=only)


ALL = [((1, 0, 1), "a single column (C = n_split)"),
       ((2, 8, 7), "T % 4 != 0: the scalar kernels"),
       ((3, 8, 36), "T % 4 == 0: the vector kernels; then each tensor in turn one float off a 16-byte boundary: scalar kernels"),
       ((300, 4, 8), "B > 256 and B > 64: the log-det fill loops, wave 3's dlogdet * x_len loop"),
       ((2, 300, 4), "C > 256: the sum(logs) loop (where n_split divides C)")]


def _all_shapes(n):
    """The shapes every kernel gets, for group size n (0: no InvConv): C becomes the nearest multiple of n."""
    res = []
    for (B, C, T), _why in ALL:
        if C == 300 and n and C % n:
            continue
        if C == 0:
            C = n or 2
        elif n and C % n:
            C = 2 * n if C == 8 else n
        res.append(pytest.param((B, C, T), n, id=f"{B}x{C}x{T}-n{n}"))
    return res


def _own(cases):
    """A kernel's own shapes: [(shape, n_split, the branch it is there for, what the library plans there)]."""
    return [pytest.param(shape, n, id="x".join(map(str, shape)) + f"-n{n}") for shape, n, _why, _plan_ in cases]


def _plan(ops, **fields):
    """What a row's prose claims, as fields of glowtts_flow_plan (and of _parent_rules' extras: items, uncapped, last) for each
    of `ops` ("coupling_fwd:rev": the reverse direction); test_plans_of_the_rows asks the library on the CPU."""
    return {op: fields for op in ops}


def _is_vec_shape(shape):
    return shape[0] == 3 and shape[2] == 36


# =============================================================================================== 1. mask_len, ActNorm
@gpu
@pytest.mark.parametrize("shape", [(1, 1), (2, 7), (3, 36), (300, 8), (3, 101)], ids=lambda s: "x".join(map(str, s)))
def test_mask_len(G, shape):
    """x_len[b] = sum_t mask[b][t] by one wave per utterance ((3, 101): a second, partial pass of the wave); 0/1 masks: exact."""
    B, T = shape
    I = _inputs("count", B, 2, T, 0)
    got = _launch(G, "mask_len", I)
    assert torch.equal(got["x_len"], I.lengths.float()), (got["x_len"], I.lengths)
    print(f"mask_len {shape}: ==")


SLAB = [((5, 1000, 12), 0, "slab_size: nbk = 3, nb = 2: three slabs of utterances, the last holds one",
         _plan(("actnorm_bwd", "actnorm_stats"), width=4, grid_x=1000, grid_y=3, nb=2, last=1)),
        ((3, 2100, 101), 0, "one slab of 303 items > 256: the item loop of a workgroup wraps",
         _plan(("actnorm_bwd", "actnorm_stats"), width=1, grid_x=2100, grid_y=1, nb=3, items=303))]


@gpu
@pytest.mark.parametrize("shape,n", _all_shapes(0))
def test_actnorm_fwd(G, shape, n):
    """glowtts_actnorm_fwd forward (with its log-det) and reverse."""
    _run(G, "actnorm_fwd", shape, revs=(False, True), misalign=_is_vec_shape(shape))


@gpu
@pytest.mark.parametrize("shape,n", _all_shapes(0) + _own(SLAB))
def test_actnorm_bwd(G, shape, n):
    """dx, dlogs (with the dlogdet * x_len term exactly once per channel, and without dlogdet), dbias; on (3, 8, 36) also added
    to a running sum, the documented contract of the accumulated outputs."""
    _run(G, "actnorm_bwd", shape, dlds=(True, False), misalign=_is_vec_shape(shape), running_sum=_is_vec_shape(shape))


@gpu
@pytest.mark.parametrize("shape,n", _all_shapes(0) + _own(SLAB))
def test_actnorm_stats(G, shape, n):
    """sum x mask and sum x^2 mask per channel (the data-dependent initialisation, oracle.actnorm_init_stats, takes its mean and
    variance from exactly these two sums and the mask count)."""
    _run(G, "actnorm_stats", shape, misalign=_is_vec_shape(shape), running_sum=_is_vec_shape(shape))
    if shape == (3, 8, 36):                                   # the two sums are what oracle.actnorm_init_stats needs
        I = _inputs("random", *shape, 0)
        got = _launch(G, "actnorm_stats", I)
        denom = I.mask.double().sum()
        m, msq = got["sum_x"].double() / denom, got["sum_x2"].double() / denom
        half_logv = 0.5 * torch.log(torch.clamp_min(msq - m * m, 1e-6))
        logs, bias = _O().actnorm_init_stats(I.x.double(), I.mask.double()[:, None])
        assert torch.allclose(-half_logv, logs.reshape(-1), rtol=0, atol=1e-5) and torch.allclose(-m * torch.exp(-half_logv), bias.reshape(-1), rtol=0, atol=1e-5)


# =============================================================================================== 2. InvConvNear
IC_BWD = [((4, 8, 16387), 2, "262192 items > 1024 x 256: the grid-stride loop of invconv_bwd_kernel runs twice, the second pass partial",
           _plan(("invconv_bwd",), width=1, n=2, items=262192, uncapped=1025, grid_x=1024, grid_y=1, launches=1))]
IC_GEN = [((2, 12, 43691), 6, "1048584 items > 4096 x 256: the workgroup cap of invconv_mix_generic_kernel",
           {**_plan(("invconv_fwd",), width=1, n=0, items=1048584, uncapped=4097, grid_x=4096, grid_y=1, launches=1, grid2_x=0),
            **_plan(("invconv_bwd",), width=1, n=0, items=1048584, uncapped=4097, grid_x=4096, grid_y=1, launches=2, grid2_x=36)})]
IC_SHAPES = [p for n in (2, 4, 8, 6, 32) for p in _all_shapes(n)]


@gpu
@pytest.mark.parametrize("shape,n", IC_SHAPES + _own(IC_GEN))
def test_invconv_fwd(G, shape, n):
    _run(G, "invconv_fwd", shape, n, misalign=_is_vec_shape(shape))


@gpu
@pytest.mark.parametrize("shape,n", IC_SHAPES + _own(IC_BWD + IC_GEN))
def test_invconv_bwd(G, shape, n):
    """dx = W^T (dz mask) and dW with the W^-T log-det term exactly once (and not at all without dlogdet); on (3, 8, 36) dW is
    also added to a running sum."""
    _run(G, "invconv_bwd", shape, n, dlds=(True, False), misalign=_is_vec_shape(shape), running_sum=_is_vec_shape(shape))


# =============================================================================================== 3. ActNorm + InvConvNear fused
_FB = ("actnorm_invconv_bwd", "coupling_ai_bwd")
FUSED_BWD = [((3, 8, 37), 4, "111 items: one slab, most threads idle",
              _plan(_FB, width=1, n=4, grid_x=2, items=111, grid_y=1, nb=111, last=111)),
             ((3, 8, 1001), 4, "G = 2: 12 slabs of 251 items, the last of 242; slab boundaries inside utterances",
              _plan(_FB, width=1, n=4, grid_x=2, items=3003, grid_y=12, nb=251, last=242)),
             ((2, 400, 1001), 4, "G = 100: 2 slabs of 1001 items: four iterations per thread, the last partial (the prefetch hand-over)",
              _plan(_FB, width=1, n=4, grid_x=100, items=2002, grid_y=2, nb=1001, last=1001)),
             ((70, 8, 5), 4, "B > 64: wave 3's dlogdet * x_len loop",
              _plan(_FB, width=1, n=4, grid_x=2, items=350, grid_y=2, nb=175, last=175)),
             ((3, 8, 1204), 4, "T % 4 == 0, the vector kernels: 903 items, 4 slabs of 226, the last of 225; boundaries inside utterances",
              _plan(_FB, width=4, n=4, grid_x=2, items=903, grid_y=4, nb=226, last=225)),
             ((2, 400, 1032), 2, "T % 4 == 0, G = 200: one slab of 516 vector items: three iterations per thread, the last partial "
                                 "(the prefetch hand-over of the vector kernels)",
              _plan(_FB, width=4, n=2, grid_x=200, items=516, grid_y=1, nb=516, last=516))]
FUSED_SHAPES = [p for n in (2, 4) for p in _all_shapes(n)]


@gpu
@pytest.mark.parametrize("shape,n", FUSED_SHAPES)
def test_actnorm_invconv_fwd(G, shape, n):
    _run(G, "actnorm_invconv_fwd", shape, n, misalign=_is_vec_shape(shape))


@gpu
@pytest.mark.parametrize("shape,n", FUSED_SHAPES + _own(FUSED_BWD))
def test_actnorm_invconv_bwd(G, shape, n):
    """dx, dlogs, dbias and dW; on (3, 8, 36) the three sums are also added to a running sum."""
    _run(G, "actnorm_invconv_bwd", shape, n, dlds=(True, False), misalign=_is_vec_shape(shape), running_sum=_is_vec_shape(shape))


# =============================================================================================== 4. affine coupling
CPL_FWD = [((2, 8, 1027), 0, "forward: 4108 items > 16 x 256 workgroups per utterance",
            _plan(("coupling_fwd",), width=1, items=4108, uncapped=17, grid_x=16, grid_y=2)),
           ((2, 8, 4099), 0, "reverse: 16396 items > 64 x 256",
            _plan(("coupling_fwd:rev",), width=1, items=16396, uncapped=65, grid_x=64, grid_y=2))]
CPL_BWD = [((2, 8, 4099), 0, "16396 items > 64 x 256 workgroups per utterance",
            _plan(("coupling_bwd",), width=1, items=16396, uncapped=65, grid_x=64, grid_y=2))]
CPL_ALL = _all_shapes(0)


@gpu
@pytest.mark.parametrize("shape,n", CPL_ALL + _own(CPL_FWD))
def test_coupling_fwd(G, shape, n):
    """z = [x0 ; (m + e^logs' x1) mask] and its reverse; logdet[b] is ADDED to (include/glowtts_hip.h: "accumulated": the caller
    zeroes it or passes a running sum): both a zero and a non-zero starting value are used."""
    _run(G, "coupling_fwd", shape, sigs=(0, 1), revs=(False, True), kinds=("count", "countld", "random"),
         misalign=_is_vec_shape(shape), running_sum=True)


@gpu
@pytest.mark.parametrize("shape,n", CPL_ALL + _own(CPL_BWD))
def test_coupling_bwd(G, shape, n):
    _run(G, "coupling_bwd", shape, sigs=(0, 1), dlds=(True, False), misalign=_is_vec_shape(shape))


# =============================================================================================== 5. coupling + ActNorm + InvConvNear
CA_FWD = [((2, 8, 1027), 4, "2054 items > 8 x 256 workgroups per utterance",
           _plan(("coupling_ai_fwd",), width=1, n=4, items=2054, uncapped=9, grid_x=8, grid_y=2))]


@gpu
@pytest.mark.parametrize("shape,n", FUSED_SHAPES + _own(CA_FWD))
def test_coupling_actnorm_invconv_fwd(G, shape, n):
    """y, logdet_prev[b] (accumulated: zero and non-zero start) and logdet[b] (written)."""
    _run(G, "coupling_ai_fwd", shape, n, sigs=(0, 1), kinds=("count", "countld", "random"), misalign=_is_vec_shape(shape),
         running_sum=True)


@gpu
@pytest.mark.parametrize("shape,n", FUSED_SHAPES + _own(FUSED_BWD))
def test_coupling_actnorm_invconv_bwd(G, shape, n):
    """dy_prev, dout_prev, dlogs, dbias and dW; on (3, 8, 36) the three sums are also added to a running sum."""
    _run(G, "coupling_ai_bwd", shape, n, sigs=(0, 1), dlds=(True, False), misalign=_is_vec_shape(shape), running_sum=_is_vec_shape(shape))


# =============================================================================================== 6. invconv_prepare
def _gauss_jordan_signs(w64):
    """(row exchanges, negative pivots) of Gauss-Jordan elimination with partial pivoting (first row of the largest |entry|)."""
    a = w64.clone()
    n = a.shape[0]
    swaps = negs = 0
    for k in range(n):
        p = k + int(a[k:, k].abs().argmax())
        if p != k:
            a[[k, p]] = a[[p, k]]
            swaps += 1
        negs += int(a[k, k] < 0)
        a[k] = a[k] / a[k, k]
        for r in range(n):
            if r != k:
                a[r] = a[r] - a[r, k] * a[k]
    return swaps, negs


def _prepare_cases(n):
    """name -> fp32 matrix: plain; zeros on the leading diagonal (pivoting has to exchange rows); an odd number of exchanges
    together with an odd number of negative pivots (the sign flips an even number of times: det > 0); det < 0."""
    cases = {"plain": _random_w(n, 100 + n)}
    for s in range(200 + n, 400 + n):
        w = _random_w(n, s).clone()
        w[0, 0] = 0.0
        if n >= 4:
            w[1, 1] = 0.0
        if float(torch.det(w.double())) < 0:
            w[:, -1] = -w[:, -1]
        if _cond(w.double()) <= 100 and float(torch.det(w.double())) > 0:
            cases["zero-diagonal"] = w
            break
    for s in range(500 + n, 900 + n):
        w = _random_w(n, s)
        swaps, negs = _gauss_jordan_signs(w.double())
        if swaps % 2 == 1 and negs % 2 == 1:
            assert float(torch.det(w.double())) > 0
            cases["odd-swaps-negative-pivot"] = w
            break
    cases["negative-det"] = _random_w(n, 900 + n, want_det=-1)
    assert len(cases) == 4, (n, sorted(cases))
    for w in cases.values():
        assert _cond(w.double()) <= 100
    return cases


def _check_prepared(w, w_inv, logdet, what):
    w64 = w.double()
    inv64 = torch.linalg.inv(w64)
    det = float(torch.det(w64))
    tol = U * inv64.abs() + 1e-9 * float(inv64.abs().max())
    worst = float(((w_inv.double() - inv64).abs() / tol).max())
    assert worst <= 1.0, f"{what}: w_inv {worst:.2f} x its bound"
    if det < 0:
        assert math.isnan(float(logdet)), f"{what}: det < 0 has to give NaN, got {float(logdet)}"
        print(f"invconv_prepare {what}: w_inv {worst:.2f} of its bound; det < 0 -> NaN")
    else:
        ld64 = float(torch.logdet(w64))
        err, bound = abs(float(logdet) - ld64), U * abs(ld64) + 1e-9
        print(f"invconv_prepare {what}: w_inv {worst:.2f} of its bound; logdet {float(logdet)!r} want {ld64!r}, |err| {err:.2e} (bound {bound:.2e})")
        assert err <= bound, f"{what}: logdet off by {err:.3e} > {bound:.3e}"


@gpu
@pytest.mark.parametrize("n", [2, 4, 6, 8, 10, 16, 32])
def test_invconv_prepare(G, n):
    """W^-1 and log det W: n <= 8 by one wave on an 8 x 8 frame padded with the identity, n > 8 by the LDS kernel."""
    for name, w in _prepare_cases(n).items():
        D = _Dev()
        G.hip.call("glowtts_invconv_prepare", D.inp("w", w), D.out("w_inv", (n, n)), D.out("logdet_w", (1,)), n)
        got = D.finish()
        _check_prepared(w, got["w_inv"], got["logdet_w"][0], f"n={n} {name}")


@gpu
@pytest.mark.parametrize("n", [4, 10])
def test_invconv_prepare_multi(G, n):
    """Three problems in one launch, out_stride > n * n + 1: log det right behind each W^-1, the padding between problems untouched."""
    cases = _prepare_cases(n)
    ws = [cases["plain"], cases["zero-diagonal"], cases["odd-swaps-negative-pivot"]]
    stride = n * n + 1 + 5
    D = _Dev()
    ptrs = [D.inp(f"w{i}", w) for i, w in enumerate(ws)]
    table = torch.tensor(ptrs, dtype=torch.int64, device="cuda")
    G.hip.call("glowtts_invconv_prepare_multi", table.data_ptr(), D.out("res", (3, stride)), stride, 3, n)
    res = D.finish()["res"]
    assert torch.equal(table.cpu(), torch.tensor(ptrs, dtype=torch.int64))
    for i, w in enumerate(ws):
        _check_prepared(w, res[i, : n * n].reshape(n, n), res[i, n * n], f"multi n={n} problem {i}")
        assert bool((res[i, n * n + 1:] == GUARD).all()), f"padding behind problem {i} written"


# =============================================================================================== 7. what the ABI has to reject
@gpu
def test_abi_rejects_before_any_launch(G):
    """n_split = 8 on the fused entry points, C % n_split != 0, dlogdet without x_len: an error code, glowtts_last_error set, and
    no output touched.  (Every buffer has the full (B, C, T) size, so nothing could be read or written out of bounds.)"""
    lib = G.hip.load()

    def rejected(op, I, match, **patch):
        J = types.SimpleNamespace(**{**vars(I), **patch})
        D = _Dev()
        with pytest.raises(RuntimeError, match=match):
            _launch(G, op, J, D=D)
        assert re.search(match, lib.glowtts_last_error().decode())
        torch.cuda.synchronize()
        assert D.outs, op
        for name, _shape, buf, off, numel in D.outs:             # accumulated outputs were handed over as zeros
            b = buf.cpu()
            keep = b[PAD + off: PAD + off + numel]
            assert bool((keep == GUARD).all()) or bool((keep == 0.0).all()), f"{op}: output {name} touched by a rejected call"
            assert bool((b[:PAD] == GUARD).all()) and bool((b[PAD + off + numel:] == GUARD).all())

    I8 = _inputs("random", 2, 8, 7, 8)
    for op in ("actnorm_invconv_fwd", "actnorm_invconv_bwd", "coupling_ai_fwd", "coupling_ai_bwd"):
        rejected(op, I8, "n_split=8")
    I4 = _inputs("random", 2, 8, 7, 4)
    wide = dict(C=10, x=torch.randn(2, 10, 7), dz=torch.randn(2, 10, 7), out=torch.randn(2, 10, 7), logs=torch.zeros(10), bias=torch.zeros(10))
    for op in ("invconv_fwd", "invconv_bwd", "actnorm_invconv_fwd", "actnorm_invconv_bwd", "coupling_ai_fwd", "coupling_ai_bwd"):
        rejected(op, I4, "bad shape|not divisible", **wide)
    for op in ("actnorm_bwd", "invconv_bwd", "actnorm_invconv_bwd", "coupling_ai_bwd"):
        rejected(op, I4, "x_len", x_len=None)


# =============================================================================================== 8. the bound table, on the CPU
TABLE_CASES = [("actnorm_fwd", 0, {}), ("actnorm_fwd", 0, {"rev": True}), ("actnorm_bwd", 0, {}),
               ("invconv_fwd", 4, {}), ("invconv_fwd", 6, {}), ("invconv_bwd", 4, {}), ("invconv_bwd", 6, {}),
               ("actnorm_invconv_fwd", 4, {}), ("actnorm_invconv_bwd", 4, {}),
               ("coupling_fwd", 0, {}), ("coupling_fwd", 0, {"sig": 1}), ("coupling_fwd", 0, {"rev": True}), ("coupling_fwd", 0, {"rev": True, "sig": 1}),
               ("coupling_bwd", 0, {}), ("coupling_bwd", 0, {"sig": 1}),
               ("coupling_ai_fwd", 4, {}), ("coupling_ai_fwd", 4, {"sig": 1}), ("coupling_ai_bwd", 4, {}), ("coupling_ai_bwd", 4, {"sig": 1})]
TABLE_SHAPES = [(2, 8, 7), (3, 8, 36), (300, 4, 8), (3, 8, 1001), (2, 400, 1001), (2, 8, 4099)]


def _fp32_cpu_figures():
    """key -> the worst figure of plain fp32 torch on the CPU against fp64, over TABLE_CASES x TABLE_SHAPES: the 'fp32 CPU'
    column of the table in the module docstring; and the worst reduction figures in units of sum|term|: [0] of the sums that the
    kernels compute, [1] of those that go through fp32 torch.logdet or its gradient (InvConv's log-det and dW), which no kernel
    here computes (w_inv and logdet_w are arguments)."""
    figs, red = {}, [0.0, 0.0]
    for op, n, kw in TABLE_CASES:
        for B, C, T in TABLE_SHAPES:
            if n and C % n:
                continue
            I = _inputs("random", B, C, T, n)
            want, got = _ref(op, I, torch.float64, **kw), _ref(op, I, torch.float32, **kw)
            for name, (kind, key, value, scale, _extra) in want.items():
                if kind == "e":
                    figs[key] = max(figs.get(key, 0.0), _units(got[name][2], value, scale))
                else:
                    err, sc = (got[name][2].double() - value).abs(), scale.double()
                    if bool((sc > 0).any()):
                        via_logdet = int(bool(n) and name in ("logdet", "dw"))
                        red[via_logdet] = max(red[via_logdet], float((err[sc > 0] / sc[sc > 0]).max()))
    return figs, red


def test_bound_table_matches_fp32_cpu_evaluation():
    """Every element-wise bound is 4 x the fp32-CPU figure rounded up to a power of two: fig <= bound <= 16 fig (4 x, the rounding
    to a power of two, and a factor 2 for another CPU's vector width); copies have bound 0 and figure 0."""
    figs, red = _fp32_cpu_figures()
    for key, fig in sorted(figs.items()):
        print(f"fp32 CPU {key}: {fig:.2f} u (bound {BOUNDS[key]})")
    print(f"fp32 CPU reductions: {red[0]:.1e} of sum|term|; through fp32 torch.logdet: {red[1]:.1e} "
          "(the bound 1e-5 is the project's figure for the kernels' reduction structure, not a measurement)")
    assert set(figs) == set(BOUNDS)
    for key, fig in figs.items():
        bound = BOUNDS[key]
        if key == "copy":
            assert fig == 0 and bound == 0
            continue
        assert bound == 2 ** round(math.log2(bound)), key
        assert fig <= bound <= 16 * fig, (key, fig, bound)


def test_counting_inputs_are_exact_in_fp32_on_the_cpu():
    """The counting inputs give the same result in fp32 and fp64 with plain torch: what the GPU tests assert EQUAL is exact in
    fp32, whatever the order of the sums."""
    for op, n, kw in TABLE_CASES:
        if kw.get("sig"):
            continue
        for B, C, T in [(2, 8, 7), (3, 8, 36), (300, 4, 8)]:
            if n and C % n:
                continue
            I = _inputs("count", B, C, T, n)
            want, got = _ref(op, I, torch.float64, **kw), _ref(op, I, torch.float32, **kw)
            _assert_exact_range(want, (op, (B, C, T), n))
            for name in want:
                assert torch.equal(got[name][2].double(), want[name][2]), (op, name, (B, C, T))


def test_counting_matrices_tell_w_from_its_inverse_and_transpose():
    for n in (2, 4, 6, 8, 32):
        w, inv = _count_w(n, n)
        assert torch.equal(w.double() @ inv.double(), torch.eye(n, dtype=torch.float64))
        assert not torch.equal(w, w.T) and not torch.equal(w, inv) and not torch.equal(w, inv.T) and not torch.equal(inv, inv.T)
        assert abs(abs(float(torch.det(w.double()))) - 1.0) < 1e-9


# =============================================================================================== 9. what the library plans, on the CPU
PLAN_FIELDS = ("width", "n", "grid_x", "grid_y", "nb", "launches", "grid2_x")
PLAN_OPS = {"actnorm_fwd": "ACTNORM_FWD", "actnorm_bwd": "ACTNORM_BWD", "actnorm_stats": "ACTNORM_STATS", "invconv_fwd": "INVCONV_FWD",
            "invconv_bwd": "INVCONV_BWD", "actnorm_invconv_fwd": "ACTNORM_INVCONV_FWD", "actnorm_invconv_bwd": "ACTNORM_INVCONV_BWD",
            "coupling_fwd": "COUPLING_FWD", "coupling_bwd": "COUPLING_BWD", "coupling_ai_fwd": "COUPLING_ACTNORM_INVCONV_FWD",
            "coupling_ai_bwd": "COUPLING_ACTNORM_INVCONV_BWD"}
_IC_OPS, _FUSED_OPS = ("invconv_fwd", "invconv_bwd"), ("actnorm_invconv_fwd", "actnorm_invconv_bwd", "coupling_ai_fwd", "coupling_ai_bwd")


def _parent_rules(op, B, C, T, n, rev, aligned):
    """What the launcher behind `op` decided while the rules stood inline in the launchers of flows.hip (the commit before
    csrc/flow_plan.hpp), restated from those launchers: None where the entry point rejects the shape, else (the plan's fields in
    the order of PLAN_FIELDS, {items, uncapped, last}: the figures the rows' prose speaks of)."""
    cdiv = lambda a, b: -(-a // b)
    if op in _IC_OPS and not (n >= 2 and n % 2 == 0 and n <= 32):
        return None
    if op in _FUSED_OPS and n not in (2, 4):
        return None
    if not (B >= 0 and C > 0 and T >= 0) or (op in _IC_OPS + _FUSED_OPS and C % n) or (op.startswith("coupling") and C % 2):
        return None
    if B * C * T == 0:
        return (0,) * 7, {}
    v4 = bool(aligned) and T % 4 == 0                        # can_vec4
    TV = T // 4 if v4 else T
    nn, gx, gy, nb, launches, g2, ex = 0, 0, 1, 0, 1, 0, {}
    if op == "actnorm_fwd":
        gx = cdiv(B * C * TV, 256)
    elif op in ("actnorm_bwd", "actnorm_stats"):             # slab_size
        nbk = max(1, min(B, cdiv(2048, C)))
        nb = cdiv(B, nbk)
        gx, gy = C, cdiv(B, nb)
        ex = dict(items=nb * TV, last=B - (gy - 1) * nb)
    elif op in _IC_OPS:
        if n in (2, 4, 8):
            nn, items = n, B * (C // n) * TV
            gx = cdiv(items, 256)
            if op == "invconv_bwd":
                gx = min(gx, 1024)
        else:
            items = B * C * TV
            gx = min(cdiv(items, 256), 4096)
            if op == "invconv_bwd":
                launches, g2 = 2, n * n
        ex = dict(items=items, uncapped=cdiv(items, 256))
    elif op == "actnorm_invconv_fwd":
        nn, gx = n, cdiv(B * (C // n) * TV, 256)
    elif op in ("actnorm_invconv_bwd", "coupling_ai_bwd"):   # ~200 workgroups
        G, items = C // n, B * TV
        slabs = max(1, min(cdiv(200, G), cdiv(items, 256)))
        nb = cdiv(items, slabs)
        nn, gx, gy = n, G, cdiv(items, nb)
        ex = dict(items=items, last=items - (gy - 1) * nb)
    elif op in ("coupling_fwd", "coupling_bwd", "coupling_ai_fwd"):
        items = (C // n if op == "coupling_ai_fwd" else C // 2) * TV
        cap = 8 if op == "coupling_ai_fwd" else 64 if (rev or op == "coupling_bwd") else 16
        nn = n if op == "coupling_ai_fwd" else 0
        gx, gy = min(cdiv(items, 256), cap), B
        ex = dict(items=items, uncapped=cdiv(items, 256))
    else:
        raise KeyError(op)
    return (4 if v4 else 1, nn, gx, gy, nb, launches, g2), ex


@functools.lru_cache(maxsize=1)
def _planner():
    import ctypes

    from glow_tts_train import _hip

    lib = _hip.load()
    out = _hip.FlowPlan()
    ref, fn = ctypes.byref(out), lib.glowtts_flow_plan_for
    codes = {op: _hip.CONSTANTS["GLOWTTS_FLOW_" + c] for op, c in PLAN_OPS.items()}
    assert sorted(codes.values()) == list(range(1, 12)) and [f for f, _ in _hip.FlowPlan._fields_] == list(PLAN_FIELDS)

    def ask(op, B, C, T, n, rev, aligned):
        """The library's plan as a tuple in the order of PLAN_FIELDS, or None where it refuses (with its error set)."""
        if fn(codes[op], B, C, T, n, rev, aligned, ref) != 0:
            assert lib.glowtts_last_error().decode().startswith("glowtts_flow_plan_for: ")
            return None
        return (out.width, out.n, out.grid_x, out.grid_y, out.nb, out.launches, out.grid2_x)

    return ask


PLAN_ROWS = SLAB + IC_BWD + IC_GEN + FUSED_BWD + CPL_FWD + CPL_BWD + CA_FWD


def test_plans_of_the_rows():
    """glowtts_flow_plan_for (no device is touched) for every own-shape row: the plan fields the row claims, and the figures its
    prose names (items, the grid before its cap, the size of the last slab), which are computed from the launch rules as they
    stood in the launchers.  A cap or a slab rule that moves fails here, on the row that no longer covers its branch."""
    ask = _planner()
    asked = 0
    for (B, C, T), n, why, claims in PLAN_ROWS:
        assert claims, why
        for key, claim in claims.items():
            op, rev = key.partition(":")[0], int(key.endswith(":rev"))
            got = ask(op, B, C, T, n, rev, 1)
            want, extras = _parent_rules(op, B, C, T, n, rev, 1)
            assert got is not None, (key, (B, C, T), n)
            named = {**dict(zip(PLAN_FIELDS, got)), **extras}
            for field, value in claim.items():
                assert named[field] == value, (key, (B, C, T), n, field, named[field], value, why)
            assert got == want, (key, (B, C, T), n, got, want)
            if "uncapped" in claim:
                assert claim["uncapped"] == claim["grid_x"] + 1, "a capped row sits right behind its cap"
            asked += 1
    assert asked == 2 * 2 + 1 + 2 + 6 * 2 + 2 + 1 + 1


def test_plans_of_the_shapes_every_kernel_gets():
    """Every ALL shape, for every operation and group size it is run with: the library's plan is the launchers' former decision;
    (2, x, 7) plans the scalar kernels, (3, x, 36) the vector kernels, and the scalar ones once a tensor is off a 16-byte boundary
    (aligned = 0); 2 / 4 / 8 plan the register kernels, 6 and 32 the run-time-N ones; one launch but for their backward."""
    ask = _planner()
    for op in PLAN_OPS:
        ns = (2, 4, 8, 6, 32) if op in _IC_OPS else (2, 4) if op in _FUSED_OPS else (0,)
        for n in ns:
            for param in _all_shapes(n):
                (B, C, T), _n = param.values
                for rev in ((0, 1) if op in ("actnorm_fwd", "coupling_fwd") else (0,)):
                    for aligned in (1, 0):
                        got = ask(op, B, C, T, n, rev, aligned)
                        assert got == _parent_rules(op, B, C, T, n, rev, aligned)[0], (op, (B, C, T), n, rev, aligned, got)
                        plan = dict(zip(PLAN_FIELDS, got))
                        assert plan["width"] == (4 if aligned and T % 4 == 0 else 1)
                        if T == 36:
                            assert plan["width"] == (4 if aligned else 1), "(3, 8, 36): vector kernels, scalar once misaligned"
                        if T == 7:
                            assert plan["width"] == 1
                        assert plan["n"] == (n if n in (2, 4, 8) else 0)
                        assert plan["launches"] == (2 if op == "invconv_bwd" and n in (6, 32) else 1)
                        assert plan["grid2_x"] == (n * n if plan["launches"] == 2 else 0)
                        assert plan["grid_x"] >= 1 and plan["grid_y"] >= 1


SWEEP_T = sorted(set(range(1, 41)) | {T for (_B, _C, T), _n, _why, _claims in PLAN_ROWS})
SWEEP_B = list(range(1, 71)) + [300]


def test_no_launch_decision_moved():
    """The library's plan against _parent_rules for every operation, n_split in 0, 2, 4, 6, 8, 32, both directions and both
    alignment verdicts over B in 1..70 and 300, C = the multiples of n_split (of 2 without groups) up to 400 and 2100, T in 1..40
    and the rows' lengths.  The full product is 10^8 questions, so it is walked along its axes: every (B, T) pair at five channel
    counts (the smallest two, G = 100 or C near 200, the largest up to 400 — ceil(200 / G) changes for the last time at G = 100
    and 200 — and 2100), and every channel count at ten (B, T) pairs with the rows' among them.  Rejections (n_split the
    operation does not take, C no multiple of it, odd C for the coupling) are compared at a few shapes."""
    ask = _planner()
    asked = 0
    for op in PLAN_OPS:
        grouped = op in _IC_OPS + _FUSED_OPS
        revs = (0, 1) if op in ("actnorm_fwd", "coupling_fwd") else (0,)
        for n in (0, 2, 4, 6, 8, 32):
            takes_n = _parent_rules(op, 1, 64, 1, n, 0, 1) is not None
            for C in (63, 64, 66):                            # rejections: agree on a few shapes, whatever n_split is
                for rev in (0, 1):
                    want = _parent_rules(op, 2, C, 8, n, rev, 1)
                    assert ask(op, 2, C, 8, n, rev, 1) == (None if want is None else want[0]), (op, C, n)
            assert ask(op, -1, 64, 8, n, 0, 1) is None and ask(op, 2, 0, 8, n, 0, 1) is None and ask(op, 2, 64, -1, n, 0, 1) is None
            if not takes_n or (not grouped and n not in (0, 6)):     # n_split is not read without groups: 0 and one other value
                continue
            step = n if grouped else 2
            all_c = list(range(step, 401, step)) + [2100 if 2100 % step == 0 else 2100 - 2100 % step]
            some_c = sorted({step, 2 * step, 100 * step if 100 * step <= 400 else 200 - 200 % step, all_c[-2], all_c[-1]})
            some_bt = [(1, 1), (2, 7), (3, 36), (5, 12), (3, 101), (70, 5), (2, 1001), (3, 1204), (2, 4099), (300, 8)]
            for rev in revs:
                for aligned in (1, 0):
                    for C in some_c:
                        for B in SWEEP_B:
                            for T in SWEEP_T:
                                if ask(op, B, C, T, n, rev, aligned) != _parent_rules(op, B, C, T, n, rev, aligned)[0]:
                                    raise AssertionError((op, (B, C, T), n, rev, aligned, ask(op, B, C, T, n, rev, aligned),
                                                          _parent_rules(op, B, C, T, n, rev, aligned)[0]))
                        asked += len(SWEEP_B) * len(SWEEP_T)
                    for C in all_c:
                        for B, T in some_bt:
                            assert ask(op, B, C, T, n, rev, aligned) == _parent_rules(op, B, C, T, n, rev, aligned)[0], (op, (B, C, T), n, rev, aligned)
                        asked += len(some_bt)
    print(f"{asked} plans compared")
    assert asked > 9 * 10 ** 5


def test_plan_for_rejects_and_empties():
    """The argument errors of the entry points come back as an error code with glowtts_last_error set; an empty tensor plans
    nothing (all fields 0), as the entry points launch nothing for it."""
    import ctypes

    from glow_tts_train import _hip

    ask, lib = _planner(), _hip.load()
    for op, n, shape, match in (("actnorm_invconv_fwd", 8, (2, 8, 7), "n_split=8"), ("coupling_ai_bwd", 8, (2, 8, 7), "n_split=8"),
                                ("invconv_fwd", 34, (2, 68, 7), "n_split=34"), ("invconv_bwd", 3, (2, 9, 7), "n_split=3"),
                                ("invconv_fwd", 4, (2, 10, 7), "not divisible"), ("coupling_ai_fwd", 4, (2, 10, 7), "bad shape"),
                                ("coupling_fwd", 0, (2, 7, 7), "bad shape"), ("actnorm_bwd", 0, (2, 0, 7), "bad shape")):
        assert ask(op, *shape, n, 0, 1) is None and re.search(match, lib.glowtts_last_error().decode()), (op, n, shape)
    out = _hip.FlowPlan()
    assert lib.glowtts_flow_plan_for(12, 2, 8, 7, 4, 0, 1, ctypes.byref(out)) != 0 and lib.glowtts_flow_plan_for(0, 2, 8, 7, 4, 0, 1, ctypes.byref(out)) != 0
    assert lib.glowtts_flow_plan_for(1, 2, 8, 7, 4, 0, 1, None) != 0
    for op in PLAN_OPS:
        n = 2 if op in _IC_OPS + _FUSED_OPS else 0
        for shape in ((0, 8, 7), (2, 8, 0)):
            assert ask(op, *shape, n, 0, 1) == (0,) * 7, (op, shape)
