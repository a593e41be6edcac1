"""The convolution family one kernel at a time, through the C ABI (glow_tts_train._hip.call), against plain fp64 torch on the CPU:
glowtts_pack_weight, _unpack_weight_grad, _rowsum, _conv_fwd (plain, with an addend, and as backward-data), _conv_fwd_act,
_conv_gate_fwd, _conv_res_skip_fwd, _conv_gate_bwd (one and two sources), _conv_wrw and _conv_wrw2, fp32 tensors only, in two
arithmetic modes: native (glowtts_conv_math(0)) and "bf16x6+wrw" (mode 15, the packed weights split by
glowtts_conv_split_weights and bound to the calling thread).  tests/test_hip_parity.py::test_conv1d_fn_vs_torch reaches these
kernels through autograd at rtol = atol = 1e-4 and tests/test_conv_math.py at max|err| / max|ref| < 2e-5 on whole production
tiles: a dropped halo frame, a frame of the neighbouring utterance or one tap too few in a partial channel group stays below
both.  The GPU tests are marked `gpu`; the tests at the end of the module are not: they check the tables below on the CPU.

References: F.conv1d on an explicitly padded input (y[t] = sum_tap sum_k w[m][k][tap] x[k][t + tap dil - pad], any pad >= 0),
einsums over shifted inputs for the weight gradient, autograd through w = g v / ||v|| for the un-packing, all in fp64.

Packed weights are ARGUMENTS: the tests build wp_f[tap][ceil(Cin/16)][Cout][16] and wp_b[taps-1-tap][ceil(Cout/16)][Cin][16]
(zero beyond the channel count) in Python from fp64 weights rounded once, so a packing error cannot cancel against a
convolution error; glowtts_pack_weight is tested on its own against the same builder.

Every launch (_Dev): each input is a copy inside a guarded buffer and must be bit-identical afterwards; each output lives between
GUARD sentinels that must survive, and is pre-filled with GUARD (written outputs) or with its starting value (accumulated ones:
dwp, dbias, rowsum's out, dv, dg, from 0 at every shape and from a running sum of small integers at one shape per kernel).
Strided tensors (x_bs, y_bs, d_bs of a channel slice) are embedded in a buffer of random values / sentinels that must not change.
Lengths are ragged: row 0 is full and from B >= 2 on one row has length 0; inputs beyond an utterance's length hold random finite
values; every masked output there must be exactly 0 and the empty row adds nothing to a masked sum.

Two kinds of input.
  1. Counting inputs: x, d, weights, bias, addend small integers in [-2, 2], masks 0/1, keep bytes 0/1 with drop_scale = 2,
     gate_scale = 2; for conv_gate_bwd the stored tanh in {-1/2, 0, 1/2} and sigmoid in {1/4, 1/2, 3/4}.  Every partial sum is an
     integer (a dyadic number for conv_gate_bwd) below 2**24, asserted per case from the sum of absolute terms before the launch,
     hence exact in fp32 in any order: ALL outputs are asserted EQUAL to the fp64 result, in both modes (a small integer is its own
     bf16 plane 0 and its planes 1 and 2 are zero, so the six-product form is exact as well:
     test_counting_inputs_are_exact_on_the_cpu emulates the split).  conv_gate_fwd has no counting form for its activations: where
     the integer pre-activation is 0 the outputs must be exactly (acts, tanh, sigmoid) = (0, 0, 1/2); the rest is left to kind 2.
  2. Random inputs: x, d ~ N(0, 1), v ~ N (Cin taps)^-1/2, g in [0.5, 1.5], bias ~ 0.1 N.  Bounds (u = 2**-24):
       * reductions (dwp, dbias, rowsum, dv, dg): |got - want| <= 1e-5 * sum|term_i|, the project's figure for "block sum + one
         float atomic per workgroup" (tests/test_flow_kernels.py, tests/test_grad_accum.py); fp32 torch on the CPU shows at most
         3.4e-7 of sum|term| on these inputs (printed by test_bound_table_matches_fp32_cpu_evaluation);
       * element-wise outputs: per element, in units of u times the magnitude of the operands; the native bound is 4 x what plain
         fp32 torch on the CPU shows against fp64 on the same inputs (the reference alone, worst over the shape tables), rounded up
         to a power of two (the margin 4: the kernels sum in another order than torch does):
             output              scale                                                                      fp32 CPU   bound
             y (conv_fwd, _act)  (sum_tap,k |w||x| + |bias|) [gate_scale] + |addend|, [mask, drop_scale]     4.61 u     32 u
             acts                sigmoid S_tanh + |tanh| S_sigmoid                                           1.47 u      8 u
             tanh                S_tanh = S_pre (1 - tanh^2) + 2 + tanh                                      1.77 u      8 u
             sigmoid             S_sigmoid = S_pre sigmoid (1 - sigmoid) + sigmoid                           2.05 u     16 u
                                 with S_pre = (sum |w||x| + |bias|) [drop_scale] + |cond|
             x_out, skip_out     sum_k |w||acts| + |bias| + |x_in| (|skip_in|), [mask]                       4.46 u     32 u
             d_pre               sum_m |w||d_rs| times sigmoid (1 + tanh^2) or |tanh| sigmoid (1 + sigmoid)  3.47 u     16 u
             w (pack, with g)    |w|                                                                         3.27 u     16 u
             inv_norm            1 / ||v||                                                                   2.21 u     16 u
         (d_pre: 1 - tanh^2 and 1 - sigmoid are differences of 1 and a stored value, their operands have magnitude 1 + tanh^2 and
         1 + sigmoid.  tanh: every kernel of the project evaluates tanh x as 2 / (1 + e^-2x) - 1 (csrc/common.hpp fast_tanh; the
         Winograd kernel likewise), a difference of 1 + tanh and 1, so the function's own rounding is measured against 2 + tanh and
         not against |tanh|: the kernels' tanh is accurate to a few u ABSOLUTELY.  Relative to |tanh| it is not: where the
         pre-activation is a small conditioning value alone (dropped frames of the case H20-T37-both, |pre| ~ 0.005) tanh is off
         by up to 123 u |tanh|, which fp32 torch.tanh is not.)
         copies (pack without g): 0 u.  In mode 15 the bound is the native bound + 2 u: include/glowtts_hip.h gives "dropped terms
         <= 2^-24 |x w|" for bf16x6, of the nine plane products x_i w_j the three with i + j >= 3 are dropped, two of them of that
         order (x_1 w_2 and x_2 w_1; x_2 w_2 is 2^-8 of them), so a product is off by at most 2 u |x w| and a sum of products by
         at most 2 u sum|w||x| <= 2 u scale; the accumulation itself is fp32 as in the native kernels (with fewer roundings: 32
         products per MFMA instead of 4).  The epilogues are the same code in both modes.
         The CPU test at the end recomputes the fp32 column and asserts fig <= bound <= 16 fig, so a bound cannot be widened
         afterwards.  Each GPU test prints its figures (-s).

Shapes: FWD, GATE, RESSKIP, GATEBWD, WRW, WRW2, ROWSUM below: each row is the smallest shape that takes a branch of the launchers
and says which; _fwd_mirror / _wrw_mirror restate the planners' rules (csrc/conv_plan.hpp, plan_conv_fwd / plan_conv_wrw) and label
every row; test_every_branch_is_reached asserts that the labels reached are exactly the EXPECT_* lists, and
test_plans_agree_with_the_mirrors asks the library itself (glowtts_conv_plan_next: no GPU needed) what it would launch for every
row, so neither a shape that silently stops reaching its branch nor a rule moved in the C++ passes on the CPU.  B <= 8,
channels <= 384, T <= 192 throughout.
"""
import ctypes
import functools
import math
import re
import types

import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu

U = 2.0 ** -24
GUARD = -1234.5          # sentinel in front of and behind every raw-ABI output
GUARD8 = 0xA5            # the same for byte buffers
PAD = 8                  # floats of guard on each side (32 bytes: the payload stays 16-byte aligned)
F64, F32 = torch.float64, torch.float32

# element-wise bounds in u (the table of the module docstring), native arithmetic; mode 15 adds SPLIT_EXTRA
BOUNDS = {"y": 32, "acts": 8, "th": 8, "sg": 16, "rs": 32, "dpre": 16, "w": 16, "inv": 16, "copy": 0}
SPLIT_EXTRA = 2          # u: two dropped cross products of <= 2^-24 |x w| per product (module docstring)
MODES = (0, 15)


# =============================================================================================== arithmetic modes
@pytest.fixture()
def G():
    """The library handle; restores the package's arithmetic mode and unbinds the planes afterwards."""
    from glow_tts_train import _hip

    lib = _hip.load()
    before = lib.glowtts_conv_math(-1)
    ns = types.SimpleNamespace(hip=_hip, lib=lib, planes=[])
    yield ns
    lib.glowtts_conv_bind_planes(None, 0, None)
    ns.planes.clear()
    assert lib.glowtts_conv_math(before) == 0


def _set_mode(G, mode, wp_ptr=None, n=0):
    """Select the arithmetic; in a plane mode split the packed weights at wp_ptr (n floats) and bind them to this thread."""
    G.lib.glowtts_conv_bind_planes(None, 0, None)
    assert G.lib.glowtts_conv_math(mode) == 0
    if (mode & 3) and wp_ptr is not None:
        planes = torch.empty(3 * n, device="cuda", dtype=torch.int16)
        G.planes.append(planes)
        G.hip.call("glowtts_conv_split_weights", wp_ptr, n, planes.data_ptr())
        assert G.lib.glowtts_conv_bind_planes(wp_ptr, n, planes.data_ptr()) == 0


# =============================================================================================== small helpers
def _units(got, want, scale):
    """max over elements of |got - want| / (u * scale); where the scale is 0 the values must agree exactly."""
    got, want, scale = got.detach().cpu().double().reshape(-1), want.detach().double().reshape(-1), scale.detach().double().reshape(-1)
    err = (got - want).abs()
    zero = scale == 0
    assert bool((err[zero] == 0).all()), "difference where the operands are all zero"
    if bool(zero.all()):
        return 0.0
    return float((err[~zero] / (U * scale[~zero])).max())


def _red_fig(got, want, terms):
    err, sc = (got.detach().cpu().double() - want.double()).abs().reshape(-1), terms.double().reshape(-1)
    assert bool((err[sc == 0] == 0).all()), "difference where every term is 0"
    return float((err[sc > 0] / sc[sc > 0]).max()) if bool((sc > 0).any()) else 0.0


def _bits_equal(a, b):
    if a.dtype == torch.uint8:
        return a.shape == b.shape and torch.equal(a, b)
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _ragged(gen, B, T):
    """Lengths in [1, T] with row 0 full and, from two rows on, one row of length 0."""
    lengths = torch.randint(1, T + 1, (B,), generator=gen)
    lengths[0] = T
    if B >= 2:
        lengths[B // 2] = 0
    return lengths


def _mask(lengths, T):
    return (torch.arange(T)[None] < lengths[:, None]).float()


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def _ints(gen, *shape):
    return torch.randint(-2, 3, shape, generator=gen).float()


def _randn(gen, *shape):
    return torch.randn(*shape, generator=gen)


def _weight(kind, gen, cout, cin, taps, norm=True):
    """(Cout, Cin, taps) fp32 weights: small integers, or w = g v / ||v|| computed in fp64 and rounded once."""
    if kind == "count":
        return _ints(gen, cout, cin, taps)
    v = torch.randn(cout, cin, taps, generator=gen, dtype=F64) * (cin * taps) ** -0.5
    if not norm:
        return v.float()
    g = 0.5 + torch.rand(cout, generator=gen, dtype=F64)
    return (g.view(-1, 1, 1) * v / v.reshape(cout, -1).norm(dim=1).view(-1, 1, 1)).float()


def _pack_f(w):
    """wp_f[tap][ceil(Cin/16)][Cout][16] = w[o][c][tap], zero beyond Cin (include/glowtts_hip.h)."""
    cout, cin, taps = w.shape
    gi = -(-cin // 16)
    wp = torch.zeros(taps, gi * 16, cout, dtype=w.dtype)
    wp[:, :cin] = w.permute(2, 1, 0)
    return wp.reshape(taps, gi, 16, cout).permute(0, 1, 3, 2).contiguous()


def _pack_b(w):
    """wp_b[taps-1-tap][ceil(Cout/16)][Cin][16] = w[o][c][tap], zero beyond Cout."""
    cout, cin, taps = w.shape
    go = -(-cout // 16)
    wp = torch.zeros(taps, go * 16, cin, dtype=w.dtype)
    wp[:, :cout] = w.flip(2).permute(2, 0, 1)
    return wp.reshape(taps, go, 16, cin).permute(0, 1, 3, 2).contiguous()


def _conv(x, w, dil, pad):
    """y[b][m][t] = sum_tap sum_k w[m][k][tap] x[b][k][t + tap dil - pad] for t in [0, T), any pad >= 0."""
    T, halo = x.shape[-1], (w.shape[2] - 1) * dil
    return F.conv1d(F.pad(x, (pad, max(halo - pad, 0))), w, dilation=dil)[..., :T]


def _embed(t, bs, gen=None, fill=None):
    """(B, C, T) rows at batch stride bs inside a flat buffer; the gaps hold random values (inputs) or `fill` (outputs)."""
    B, C, T = t.shape
    flat = torch.randn((B - 1) * bs + C * T, generator=gen) if fill is None else torch.full(((B - 1) * bs + C * T,), fill)
    torch.as_strided(flat, (B, C * T), (bs, 1)).copy_(t.reshape(B, C * T))
    return flat


def _extract(flat, B, C, T, bs):
    """The (B, C, T) rows of a strided output and whether everything between them still holds GUARD."""
    rows = torch.as_strided(flat, (B, C * T), (bs, 1)).clone()
    rest = flat.clone()
    torch.as_strided(rest, (B, C * T), (bs, 1)).fill_(GUARD)
    return rows.reshape(B, C, T), bool((rest == GUARD).all())


# =============================================================================================== the launches
class _Dev:
    """The buffers of one raw-ABI call: inputs are copies inside guarded buffers (bit-identical afterwards), outputs live between
    GUARD sentinels.  off = 1 puts a float tensor one float off its 16-byte boundary."""

    def __init__(self):
        self.ins, self.outs = [], {}

    @staticmethod
    def _place(numel, off, dtype):
        pad = PAD if dtype == torch.float32 else 4 * PAD
        buf = torch.full((numel + 2 * pad,), GUARD if dtype == torch.float32 else GUARD8, device="cuda", dtype=dtype)
        view = buf[pad + off: pad + off + numel]
        assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == buf.element_size() * off
        return buf, view, pad + off

    def inp(self, name, t, off=0):
        if t is None:
            return None
        t = t.contiguous()
        buf, view, lo = self._place(t.numel(), off, t.dtype)
        view.copy_(t.reshape(-1))
        self.ins.append((name, t, buf, lo))
        return view.data_ptr()

    def out(self, name, numel, init=None, off=0):
        numel = int(math.prod(numel)) if not isinstance(numel, int) else numel
        buf, view, lo = self._place(numel, off, torch.float32)
        if init is not None:
            view.copy_(init.reshape(-1).float() if torch.is_tensor(init) else torch.full((numel,), float(init)))
        self.outs[name] = (buf, lo, numel)
        return view.data_ptr()

    def finish(self):
        torch.cuda.synchronize()
        for name, t, buf, lo in self.ins:
            b = buf.cpu()
            g = GUARD if t.dtype == torch.float32 else GUARD8
            assert _bits_equal(b[lo: lo + t.numel()], t.reshape(-1)), f"input {name} changed"
            assert bool((b[:lo] == g).all()) and bool((b[lo + t.numel():] == g).all()), f"written around input {name}"
        res = {}
        for name, (buf, lo, numel) in self.outs.items():
            b = buf.cpu()
            assert bool((b[:lo] == GUARD).all()) and bool((b[lo + numel:] == GUARD).all()), f"guard of output {name} overwritten"
            res[name] = b[lo: lo + numel].clone()
        return res


def _start(numel, seed):
    """A running sum of small integers, the starting value of an accumulated output."""
    return torch.randint(1, 4, (numel,), generator=_gen(numel, seed)).float()


def _check_elem(what, name, key, got, want, scale, kind, mode, figs, zero_where=None):
    assert got.shape == want.shape, (what, name, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), f"{what} {name}: non-finite output"
    if zero_where is not None:
        assert bool((got[zero_where.expand_as(got)] == 0).all()), f"{what} {name}: not exactly 0 behind an utterance's end"
    if kind == "count":
        assert torch.equal(got.double(), want.double()), \
            f"{what} {name}: differs from integer arithmetic by up to {float((got.double() - want).abs().max())} at " \
            f"{[tuple(i.tolist()) for i in (got.double() != want).nonzero()[:4]]}"
        figs.append(f"{name} ==")
        return
    bound = BOUNDS[key] + (SPLIT_EXTRA if (mode & 3) and BOUNDS[key] else 0)
    fig = _units(got, want, scale)
    figs.append(f"{name} {fig:.2f} u (bound {bound})")
    assert fig <= bound, f"{what} {name}: {fig:.2f} u > {bound} u"


def _check_red(what, name, got, want, terms, kind, figs):
    assert got.shape == want.shape, (what, name, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), f"{what} {name}: non-finite output"
    if kind == "count":
        assert torch.equal(got.double(), want.double()), \
            f"{what} {name}: differs from integer arithmetic by up to {float((got.double() - want).abs().max())} at " \
            f"{[tuple(i.tolist()) for i in (got.double() != want).nonzero()[:4]]}"
        figs.append(f"{name} ==")
        return
    fig = _red_fig(got, want, terms)
    figs.append(f"{name} {fig:.1e} of sum|term| (bound 1e-5)")
    assert fig <= 1e-5, f"{what} {name}: {fig:.2e} of sum|term| > 1e-5"


def _assert_exact(what, *scales):
    """Counting inputs: the sum of absolute terms bounds every partial sum in any order; below 2**24 all of them are exact."""
    for s in scales:
        assert float(s.abs().max()) < 2 ** 24 if s.numel() else True, what


def _case(name, why, **kw):
    return types.SimpleNamespace(name=name, why=why, **kw)


def _ids(table):
    return [pytest.param(c, id=c.name) for c in table]


# =============================================================================================== 1. forward-type convolutions
def _fwd(name, why, Cin, M, T, taps, dil=1, pad=None, B=2, **kw):
    d = dict(mask_in=0, mask_out=0, mask_add=0, addend=False, x_slice=False, y_slice=False, a_slice=False, x_bs_odd=False,
             y_bs_odd=False, mis=None, relu=0, drop=False, gate_pos=False, bwd=False, act=False)
    d.update(kw)
    d["act"] = bool(d["act"] or d["relu"] or d["drop"] or d["gate_pos"])
    return _case(name, why, B=B, Cin=Cin, M=M, T=T, taps=taps, dil=dil, pad=(taps - 1) * dil // 2 if pad is None else pad, **d)


FWD = [
    # the generic kernel, four ways
    _fwd("g-T37", "T % 4 != 0: generic kernel; Cin = 20 (partial group), M = 36 (partial 64-row tile), T < tile", 20, 36, 37, 3, B=3),
    _fwd("g-halo16", "halo (taps-1) dil = 16 > 12 with T % 4 == 0: generic kernel", 16, 16, 40, 5, dil=4),
    _fwd("g-taps2", "2 taps (even), pad 0, aligned data: generic kernel although pipe_ok", 20, 20, 40, 2, pad=0),
    _fwd("g-taps7", "7 taps, aligned data: generic kernel although pipe_ok; all masks", 20, 20, 40, 7, mask_in=1, mask_out=1),
    _fwd("g-xmis", "x one float off a 16-byte boundary: generic kernel", 16, 16, 40, 3, mis="x"),
    _fwd("g-xbs", "x_bs % 4 != 0: generic kernel", 16, 16, 40, 3, x_bs_odd=True, B=3),
    # the pipelined kernel: taps, window offsets, paddings
    _fwd("p1", "1 tap, off 0, Cin = 80, 64-frame tile larger than T", 80, 36, 40, 1),
    _fwd("p3", "3 taps, pad 1: off 3", 20, 36, 40, 3, B=3),
    _fwd("p5", "5 taps, pad 2: off 2; mode 15: PLAIN 5 taps / 64 rows", 20, 36, 40, 5),
    _fwd("p3-pad3", "3 taps at dilation 3, pad 3: off 1", 20, 36, 40, 3, dil=3),
    _fwd("p3-pad5", "3 taps at dilation 5, pad 5: off 3 with pad > 4", 20, 36, 40, 3, dil=5),
    _fwd("p3-pad0", "3 taps, pad 0 (not 'same')", 20, 36, 40, 3, pad=0),
    _fwd("p3-padh", "3 taps, pad = (taps-1) dil = 2 (not 'same')", 20, 36, 40, 3, pad=2),
    _fwd("p5-halo12", "5 taps at dilation 3: halo exactly 12, pad 6", 20, 36, 40, 5, dil=3),
    _fwd("p5-dil2", "5 taps at dilation 2, pad 4: off 0 with a halo", 20, 36, 40, 5, dil=2),
    _fwd("p3-bwd", "backward-data of a 3-tap pad-0 convolution: wp_b, pad' = (taps-1) dil - 0 = 2", 36, 20, 40, 3, pad=2, bwd=True),
    _fwd("p5-bwd", "backward-data of a 5-tap 'same' convolution with the addend (the WN input gradient)", 40, 20, 40, 5, bwd=True,
         addend=True, mask_out=1),
    # tile geometry
    _fwd("r-M8", "M < 16", 16, 8, 40, 3),
    _fwd("r-M72", "two 64-row tiles, the last partial", 16, 72, 40, 3),
    _fwd("r-M160", "three 64-row tiles, the last partial (M = 160 is neither % 128 nor > 192)", 16, 160, 40, 3),
    _fwd("r-M128", "one 128-row tile; mode 15: PLAIN 3 taps / 128 rows", 16, 128, 40, 3),
    _fwd("r-M200", "M > 192: 128-row tiles, the last partial", 16, 200, 40, 1),
    _fwd("f-T80", "80-frame tile (T % 80 == 0)", 16, 36, 80, 3),
    _fwd("f-T68", "80-frame tile, partial (ceil80 < ceil64)", 16, 36, 68, 3),
    _fwd("f-T100", "64-frame tiles, the last partial", 16, 36, 100, 3),
    _fwd("f-T64", "32-frame tiles (small grid); mode 15: PLAIN 3 taps / 32 frames", 16, 36, 64, 3),
    _fwd("f-T88", "32-frame tiles, the last partial", 16, 36, 88, 5),
    _fwd("f-T96-1x1", "1 tap: 32-frame tiles", 16, 36, 96, 1),
    # channel counts
    _fwd("c-5", "Cin < 16", 5, 36, 40, 3),
    _fwd("c-100", "Cin = 100: 7 groups, chunk 1 has one group with 4 live channels", 100, 36, 40, 3),
    _fwd("c-100-5", "the same at 5 taps", 100, 36, 40, 5),
    _fwd("c-192", "Cin = 192: two full chunks", 192, 36, 40, 3),
    # strides, masks
    _fwd("s-x", "x is the upper channel half of a (B, 2 Cin, T) tensor: x_bs = 2 Cin T", 20, 36, 40, 3, x_slice=True, B=3),
    _fwd("s-y", "y is the upper channel half of a (B, 2 M, T) tensor: y_bs = 2 M T", 20, 36, 40, 3, y_slice=True, B=3),
    _fwd("s-a", "addend and y both slices", 20, 36, 40, 5, addend=True, a_slice=True, y_slice=True, B=3),
    _fwd("m-in", "mask_in only", 20, 36, 40, 3, mask_in=1, B=3),
    _fwd("m-out", "mask_out only", 20, 36, 40, 3, mask_out=1, B=3),
    _fwd("m-add", "mask_add only; mode 15: ADD 3 taps / 64 rows", 20, 36, 40, 3, addend=True, mask_add=1, B=3),
    _fwd("m-all", "mask_in, mask_out, mask_add; mode 15: ADD 5 taps / 64 rows", 20, 36, 40, 5, addend=True, mask_in=1, mask_out=1,
         mask_add=1, B=3),
    _fwd("m-all-128", "all masks on 128 rows; mode 15: ADD 3 taps / 128 rows", 20, 128, 40, 3, addend=True, mask_in=1, mask_out=1,
         mask_add=1, B=3),
    _fwd("m-all-g", "all masks in the generic kernel (T % 4 != 0)", 20, 36, 37, 3, addend=True, mask_in=1, mask_out=1, mask_add=1, B=3),
    # the scalar epilogue of the pipelined kernel
    _fwd("e-y", "y one float off a 16-byte boundary, x aligned: scalar epilogue", 20, 36, 40, 3, mis="y", mask_out=1),
    _fwd("e-a", "addend one float off, x aligned: scalar epilogue", 20, 36, 40, 5, mis="addend", addend=True, mask_add=1),
    _fwd("e-ybs", "y_bs % 4 != 0: scalar epilogue", 20, 36, 40, 3, y_bs_odd=True, B=3),
    # conv_fwd_act
    _fwd("a-relu", "relu", 20, 36, 40, 3, relu=1),
    _fwd("a-drop", "drop", 20, 36, 40, 3, drop=True),
    _fwd("a-gate", "gate_pos", 20, 36, 40, 3, gate_pos=True),
    _fwd("a-gate-add", "gate_pos, then the addend (masked), then the mask, relu and drop: the header's order", 20, 36, 40, 3,
         gate_pos=True, addend=True, mask_add=1, mask_out=1, relu=1, drop=True, B=3),
    _fwd("a-gate-add-g", "the same in the generic kernel", 20, 36, 37, 3, gate_pos=True, addend=True, mask_add=1, mask_out=1, relu=1,
         drop=True, B=3),
    _fwd("a-plain", "conv_fwd_act with no flag set", 20, 36, 40, 1, act=True),
]


def _fwd_mirror(c):
    """The decisions of plan_conv_fwd for conv_fwd / conv_fwd_act (csrc/convgemm.hip) with the rules of csrc/conv_plan.hpp and
    conv_split_has (csrc/convgemm_split.hip) -> namespace with the labels of the case."""
    halo = (c.taps - 1) * c.dil
    x_aligned, x_bs_ok = c.mis != "x", not c.x_bs_odd                                     # fwd_pipe_ok
    pipe_ok = c.T % 4 == 0 and x_aligned and x_bs_ok and halo <= 12                       # fwd_pipe_ok (the mask is always aligned here)
    wd = pipe_ok and c.taps in (1, 3, 5)                                                  # plan_conv_fwd: PIPE or GENERIC
    n5 = c.T % 80 == 0 or (c.T % 64 != 0 and -(-c.T // 80) * 80 < -(-c.T // 64) * 64)     # frames80_fwd
    big = c.M % 128 == 0 or c.M > 192                                                     # rows_big
    epi = "ADD" if c.addend else "PLAIN"
    use32 = False
    if epi == "PLAIN" and pipe_ok:                                                        # fwd_use32
        wg5 = -(-c.T // 80) * c.B * -(-c.M // (128 if big else 64))
        t32 = -(-c.T // 32) * 32
        use32 = (wg5 < 380 and t32 * 10 <= c.T * 11) or (c.taps == 1 and t32 * 10 <= c.T * 11)
    nct = 2 if use32 else (5 if n5 else 4)                                                # plan.frame_tile
    vec = wd and c.mis not in ("y", "addend") and not c.y_bs_odd                          # vec_epilogue
    split = None                                                                          # plan_conv_fwd: SPLIT; conv_split_has
    if pipe_ok:
        if c.taps == 5 and not big and nct != 2:
            split = f"{epi}5/64"
        elif c.taps == 3 and nct != 2:
            split = f"{epi}3/{128 if big else 64}"
        elif c.taps == 3 and nct == 2 and epi == "PLAIN" and not big:
            split = "PLAIN3/32f"
    L = set()
    if not wd:
        L.add("generic:T%4" if c.T % 4 else "generic:halo>12" if halo > 12 else "generic:x-misaligned" if not x_aligned
              else "generic:x_bs%4" if not x_bs_ok else f"generic:taps{c.taps}")
    else:
        L |= {f"pipe:taps{c.taps}", f"off{(4 - (c.pad & 3)) & 3}"}
        L |= {"pad3"} if c.pad == 3 else {"pad5"} if c.pad == 5 else set()
        if c.taps > 1 and not c.bwd:
            L |= {"pad:0"} if c.pad == 0 else {"pad:halo"} if c.pad == halo else set()
        L |= {"halo12"} if halo == 12 else set()
        if not vec:
            L.add("scalar-epilogue:" + ("y" if c.mis == "y" or c.y_bs_odd else "addend"))
    rows, nt = (128 if big else 64), 16 * nct
    L |= {f"rows{rows}", f"nt{nt}"}
    L |= {"partial-row-tile"} if c.M % rows else set()
    L |= {"M<16"} if c.M < 16 else set()
    L |= {"T<tile"} if c.T < nt else {"partial-frame-tile"} if c.T % nt else set()
    L |= {"Cin<16"} if c.Cin < 16 else {f"Cin{c.Cin}"} if c.Cin in (80, 100, 192) else set()
    L |= {"x-slice"} if c.x_slice else set()
    L |= {"y-slice"} if c.y_slice else set()
    masks = (c.mask_in, c.mask_out, c.mask_add)
    L |= {"mask-all"} if all(masks) else {n for n, f in zip(("mask_in", "mask_out", "mask_add"), masks) if f and sum(masks) == 1}
    if c.gate_pos and c.addend and c.mask_out and c.mask_add:
        L.add("gate_pos+addend+mask")
    else:
        L |= {n for n in ("relu", "drop", "gate_pos") if getattr(c, n) and sum(map(bool, (c.relu, c.drop, c.gate_pos))) == 1}
    L |= {"bwd-data"} if c.bwd else set()
    L.add("split:" + (split or "none"))
    wg5 = -(-c.T // 80) * c.B * -(-c.M // rows)
    return types.SimpleNamespace(pipe_ok=pipe_ok, wd=wd, n5=n5, big=big, use32=use32, vec=vec, split=split, labels=L, wg5=wg5)


EXPECT_FWD = {
    "generic:T%4", "generic:halo>12", "generic:taps2", "generic:taps7", "generic:x-misaligned", "generic:x_bs%4",
    "pipe:taps1", "pipe:taps3", "pipe:taps5", "off0", "off1", "off2", "off3", "pad3", "pad5", "pad:0", "pad:halo", "halo12",
    "rows64", "rows128", "partial-row-tile", "M<16", "nt80", "nt64", "nt32", "partial-frame-tile", "T<tile",
    "Cin<16", "Cin80", "Cin100", "Cin192", "x-slice", "y-slice", "mask_in", "mask_out", "mask_add", "mask-all",
    "scalar-epilogue:y", "scalar-epilogue:addend", "relu", "drop", "gate_pos", "gate_pos+addend+mask", "bwd-data",
    "split:PLAIN5/64", "split:ADD5/64", "split:PLAIN3/64", "split:PLAIN3/128", "split:ADD3/64", "split:ADD3/128", "split:PLAIN3/32f",
    "split:none"}


@functools.lru_cache(maxsize=None)
def _fwd_inputs(name, kind):
    c = next(c for c in FWD if c.name == name)
    gen = _gen(len(name), sum(map(ord, name)), c.Cin, c.M, c.T, len(kind))
    r = (lambda *s: _ints(gen, *s)) if kind == "count" else (lambda *s: _randn(gen, *s))
    I = types.SimpleNamespace(kind=kind)
    I.lengths = _ragged(gen, c.B, c.T)
    I.mask = _mask(I.lengths, c.T)
    I.x = r(c.B, c.Cin, c.T)
    if c.bwd:     # the convolution whose input gradient this is maps M -> Cin channels; its wp_b is what the kernel gets
        I.w_orig = _weight(kind, gen, c.Cin, c.M, c.taps)
        I.w, I.wp = I.w_orig.transpose(0, 1).flip(2).contiguous(), _pack_b(I.w_orig)
    else:
        I.w = _weight(kind, gen, c.M, c.Cin, c.taps)
        I.wp = _pack_f(I.w)
    I.bias = r(c.M) if kind == "count" else 0.1 * r(c.M)
    I.addend = r(c.B, c.M, c.T) if c.addend else None
    I.drop = (torch.rand(c.B, c.M, c.T, generator=gen) < 0.7).to(torch.uint8) if c.drop else None
    I.gate_pos = (r(c.B, c.M, c.T) if kind == "count" else r(c.B, c.M, c.T).clamp_min(0.0)) if c.gate_pos else None
    I.drop_scale, I.gate_scale = (2.0, 2.0) if kind == "count" else (1.0 / 0.7, 1.25)
    return I


def _fwd_ref(c, I, dt):
    """(y, scale) of conv_fwd / conv_fwd_act in dtype dt, in the order of include/glowtts_hip.h."""
    t = lambda a: None if a is None else a.to(dt)
    x, w, bias, m = t(I.x), t(I.w), t(I.bias), t(I.mask)[:, None]
    xm = x * m if c.mask_in else x
    y = _conv(xm, w, c.dil, c.pad) + bias.view(1, -1, 1)
    s = _conv(xm.abs(), w.abs(), c.dil, c.pad) + bias.abs().view(1, -1, 1)
    if c.gate_pos:
        pos = I.gate_pos > 0
        y, s = torch.where(pos, y * I.gate_scale, torch.zeros_like(y)), torch.where(pos, s * I.gate_scale, torch.zeros_like(s))
    if c.addend:
        a = t(I.addend) * m if c.mask_add else t(I.addend)
        y, s = y + a, s + a.abs()
    if c.mask_out:
        y, s = y * m, s * m
    if c.relu:
        y = torch.relu(y)
    if c.drop:
        keep = I.drop.bool()
        y, s = torch.where(keep, y * I.drop_scale, torch.zeros_like(y)), torch.where(keep, s * I.drop_scale, torch.zeros_like(s))
    return y, s


def _fwd_launch(G, c, I, mode, arm=None):
    """arm: a ConvPlan — glowtts_conv_plan_next(arm) right before the call, which then must launch nothing."""
    D = _Dev()
    B, Cin, M, T = c.B, c.Cin, c.M, c.T
    gen = _gen(B, Cin, M, T)
    if c.x_slice:
        x_bs, x_ptr = 2 * Cin * T, D.inp("x", torch.cat([_randn(gen, B, Cin, T), I.x], 1)) + 4 * Cin * T
    else:
        x_bs = Cin * T + (2 if c.x_bs_odd else 0)
        x_ptr = D.inp("x", _embed(I.x, x_bs, gen), off=int(c.mis == "x"))
    a_ptr, a_bs = None, 0
    if c.addend:
        if c.a_slice:
            a_bs, a_ptr = 2 * M * T, D.inp("addend", torch.cat([I.addend, _randn(gen, B, M, T)], 1))
        else:
            a_bs, a_ptr = M * T, D.inp("addend", I.addend, off=int(c.mis == "addend"))
    y_bs = 2 * M * T if c.y_slice else M * T + (2 if c.y_bs_odd else 0)
    y_base = D.out("y", (B - 1) * y_bs + (2 if c.y_slice else 1) * M * T, off=int(c.mis == "y"))
    y_ptr = y_base + (4 * M * T if c.y_slice else 0)
    wp_ptr = D.inp("wp", I.wp)
    any_mask = c.mask_in or c.mask_out or c.mask_add
    args = [x_ptr, x_bs, wp_ptr, D.inp("bias", I.bias), D.inp("mask", I.mask) if any_mask else None, a_ptr, a_bs, y_ptr, y_bs,
            B, Cin, M, T, c.taps, c.dil, c.pad, c.mask_in, c.mask_out, c.mask_add]
    _set_mode(G, mode, wp_ptr, I.wp.numel())
    if arm is not None:
        assert G.lib.glowtts_conv_plan_next(ctypes.byref(arm)) == 0
    if c.act:
        G.hip.call("glowtts_conv_fwd_act", *args, c.relu, D.inp("drop", I.drop), I.drop_scale, D.inp("gate_pos", I.gate_pos), I.gate_scale)
    else:
        G.hip.call("glowtts_conv_fwd", *args)
    flat = D.finish()["y"]
    y, clean = _extract(flat[M * T:] if c.y_slice else flat, B, M, T, y_bs)
    assert clean and (not c.y_slice or bool((flat[:M * T] == GUARD).all())), "written between the rows of the strided output"
    return y


@gpu
@pytest.mark.parametrize("c", _ids(FWD))
def test_conv_fwd(G, c):
    """glowtts_conv_fwd / glowtts_conv_fwd_act at one row of FWD, counting and random inputs, native and mode 15.  Where the mirror
    finds no bf16-plane instantiation the mode-15 result must equal the native one bit for bit; where it finds one, the random
    result must differ from the native one (the plane kernel really ran)."""
    mir = _fwd_mirror(c)
    for kind in ("count", "random"):
        I = _fwd_inputs(c.name, kind)
        behind = (I.mask == 0)[:, None] if c.mask_out else None
        want, scale = _fwd_ref(c, I, F64)
        if kind == "count":
            _assert_exact(c.name, scale)
        got = {}
        for mode in MODES:
            figs = []
            got[mode] = _fwd_launch(G, c, I, mode)
            _check_elem(f"conv_fwd {c.name} {kind} mode {mode}", "y", "y", got[mode], want, scale, kind, mode, figs, behind)
            print(f"conv_fwd {c.name} {kind} mode {mode} [{' '.join(sorted(mir.labels))}]: " + "; ".join(figs))
        if mir.split is None:
            assert _bits_equal(got[0], got[15]), f"{c.name}: no bf16-plane kernel for this shape, yet mode 15 differs from native"
        elif kind == "random":
            assert not _bits_equal(got[0], got[15]), f"{c.name}: the mirror expects the bf16-plane kernel {mir.split}, the result is native"


# =============================================================================================== 2. gated in-conv
def _gate(name, why, H, T, taps, dil=1, B=2, cond=False, drop=False, ts_null=False):
    return _case(name, why, B=B, H=H, T=T, taps=taps, dil=dil, pad=(taps - 1) * dil // 2, cond=cond, drop=drop, ts_null=ts_null)


GATE = [
    _gate("H20-3", "H = 20: partial 64-row halves, 3 taps", 20, 40, 3, B=3),
    _gate("H20-T37", "T % 4 != 0: generic kernel", 20, 37, 3, B=3),
    _gate("H20-dil2", "dilation 2", 20, 40, 3, dil=2),
    _gate("H20-5-cond", "5 taps, cond", 20, 40, 5, cond=True),
    _gate("H20-5-drop", "drop", 20, 40, 5, drop=True),
    _gate("H20-5-both", "cond and drop: the dropout acts on conv + bias, cond is added afterwards", 20, 40, 5, cond=True, drop=True),
    _gate("H20-T37-both", "the same in the generic kernel's scalar epilogue", 20, 37, 5, cond=True, drop=True),
    _gate("H96-5", "H = 96", 96, 40, 5),
    _gate("H192-5", "H = 192, two chunks, 80-frame tile", 192, 80, 5),
    _gate("H96-3-nots", "ts == NULL (documented: 'or null')", 96, 40, 3, ts_null=True),
]
EXPECT_GATE = {"H20", "H96", "H192", "taps3", "taps5", "dil2", "generic:T%4", "pipe", "cond", "drop", "cond+drop", "ts-null",
               "split:GATE5", "split:none"}


def _gate_mirror(c):
    pipe_ok = c.T % 4 == 0 and (c.taps - 1) * c.dil <= 12 and c.H % 4 == 0                # fwd_pipe_ok
    split = "GATE5" if pipe_ok and c.taps == 5 else None                                  # conv_split_has (EPI_GATE is always `big`)
    L = {f"H{c.H}", f"taps{c.taps}", "pipe" if pipe_ok and c.taps in (1, 3, 5) else "generic:T%4", "split:" + (split or "none")}
    L |= {"dil2"} if c.dil == 2 else set()
    L |= {"cond+drop"} if c.cond and c.drop else {"cond"} if c.cond else {"drop"} if c.drop else set()
    L |= {"ts-null"} if c.ts_null else set()
    return types.SimpleNamespace(split=split, labels=L)


@functools.lru_cache(maxsize=None)
def _gate_inputs(name, kind):
    c = next(c for c in GATE if c.name == name)
    gen = _gen(c.H, c.T, c.taps, c.dil, len(kind), len(name))
    r = (lambda *s: _ints(gen, *s)) if kind == "count" else (lambda *s: _randn(gen, *s))
    I = types.SimpleNamespace(kind=kind)
    I.x = r(c.B, c.H, c.T)
    I.w = _weight(kind, gen, 2 * c.H, c.H, c.taps)
    I.wp = _pack_f(I.w)
    I.bias = r(2 * c.H) if kind == "count" else 0.1 * r(2 * c.H)
    I.cond = (r(c.B, 2 * c.H) if kind == "count" else 0.5 * r(c.B, 2 * c.H)) if c.cond else None
    I.drop = (torch.rand(c.B, 2 * c.H, c.T, generator=gen) < 0.7).to(torch.uint8) if c.drop else None
    I.drop_scale = 2.0 if kind == "count" else 1.0 / 0.7
    return I


def _gate_ref(c, I, dt):
    """name -> (key, value, scale) of conv_gate_fwd, and the pre-activation."""
    t = lambda a: None if a is None else a.to(dt)
    pre = _conv(t(I.x), t(I.w), c.dil, c.pad) + t(I.bias).view(1, -1, 1)
    s = _conv(t(I.x).abs(), t(I.w).abs(), c.dil, c.pad) + t(I.bias).abs().view(1, -1, 1)
    if c.drop:
        keep = I.drop.bool()
        pre, s = torch.where(keep, pre * I.drop_scale, torch.zeros_like(pre)), torch.where(keep, s * I.drop_scale, torch.zeros_like(s))
    if c.cond:
        pre, s = pre + t(I.cond)[:, :, None], s + t(I.cond).abs()[:, :, None]
    th, sg = torch.tanh(pre[:, :c.H]), torch.sigmoid(pre[:, c.H:])
    # tanh is 2 / (1 + e^-2x) - 1 in every kernel of the project (csrc/common.hpp fast_tanh, csrc/convwino.hip): the operands of its
    # last operation are 1 + tanh and 1; sigmoid is 1 / (1 + e^-x), a quotient: its own magnitude
    s_th, s_sg = s[:, :c.H] * (1 - th * th) + (2 + th), s[:, c.H:] * sg * (1 - sg) + sg
    return {"acts": ("acts", th * sg, sg * s_th + th.abs() * s_sg), "th": ("th", th, s_th), "sg": ("sg", sg, s_sg)}, pre


@gpu
@pytest.mark.parametrize("c", _ids(GATE))
def test_conv_gate_fwd(G, c):
    """acts = tanh(pre[:H]) sigmoid(pre[H:]) and ts = [tanh ; sigmoid], pre = dropout(conv(x) + bias) + cond.  Counting inputs:
    exactly (0, 0, 1/2) wherever the integer pre-activation is 0; random inputs: the bounds of the module docstring."""
    mir = _gate_mirror(c)
    B, H, T = c.B, c.H, c.T
    for kind in ("count", "random"):
        I = _gate_inputs(c.name, kind)
        want, pre = _gate_ref(c, I, F64)
        got = {}
        for mode in MODES:
            D = _Dev()
            wp_ptr = D.inp("wp", I.wp)
            args = [D.inp("x", I.x), wp_ptr, D.inp("bias", I.bias), D.inp("cond", I.cond), D.inp("drop", I.drop), I.drop_scale,
                    D.out("acts", B * H * T), None if c.ts_null else D.out("ts", B * 2 * H * T), B, H, T, c.taps, c.dil, c.pad]
            _set_mode(G, mode, wp_ptr, I.wp.numel())
            G.hip.call("glowtts_conv_gate_fwd", *args)
            r = D.finish()
            out = {"acts": r["acts"].reshape(B, H, T)}
            if not c.ts_null:
                ts = r["ts"].reshape(B, 2 * H, T)
                out["th"], out["sg"] = ts[:, :H], ts[:, H:]
            got[mode] = out
            figs = []
            for name, g in out.items():
                key, value, scale = want[name]
                assert bool(torch.isfinite(g).all()), (c.name, name)
                if kind == "count":
                    z_t, z_s = pre[:, :H] == 0, pre[:, H:] == 0
                    assert int(z_t.sum()) > 0 and int(z_s.sum()) > 0, "no zero pre-activation in the counting inputs"
                    zero, val = {"acts": (z_t, 0.0), "th": (z_t, 0.0), "sg": (z_s, 0.5)}[name]
                    assert bool((g[zero] == val).all()), f"conv_gate_fwd {c.name} {name}: a zero pre-activation does not give exactly {val}"
                    assert float((g.double() - value).abs().max()) < 1e-3, f"conv_gate_fwd {c.name} {name}: wrong pre-activation"
                    figs.append(f"{name} == at {int(zero.sum())} zeros")
                else:
                    _check_elem(f"conv_gate_fwd {c.name} mode {mode}", name, key, g, value, scale, kind, mode, figs)
            print(f"conv_gate_fwd {c.name} {kind} mode {mode} [{' '.join(sorted(mir.labels))}]: " + "; ".join(figs))
        same = all(_bits_equal(got[0][n], got[15][n]) for n in got[0])
        if mir.split is None:
            assert same, f"{c.name}: no bf16-plane kernel for this shape, yet mode 15 differs from native"
        elif kind == "random":
            assert not same, f"{c.name}: the mirror expects the bf16-plane kernel, the result is native"


# =============================================================================================== 3. res/skip 1x1
def _rs(name, why, H, T, last, B=2, skip_null=False, alias=False, xout_null=False):
    return _case(name, why, B=B, H=H, T=T, last=last, skip_null=skip_null, alias=alias, xout_null=xout_null)


RESSKIP = [
    _rs("H20", "H = 20, 64-row tile of 40 rows", 20, 40, 0, B=3),
    _rs("H20-T37", "T % 4 != 0: generic kernel", 20, 37, 0, B=3),
    _rs("H20-last", "last, H = 20; mode 15: RESSKIP_LAST", 20, 40, 1, B=3),
    _rs("H20-last-T37", "last in the generic kernel", 20, 37, 1, B=3),
    _rs("H96", "H = 96: 192 rows in 64-row tiles (no bf16-plane instantiation)", 96, 40, 0),
    _rs("H96-noskip", "skip_in == NULL", 96, 40, 0, skip_null=True),
    _rs("H96-last", "last, H = 96; mode 15: RESSKIP_LAST (64-row)", 96, 40, 1),
    _rs("H192", "H = 192: 384 rows in 128-row tiles; mode 15: RESSKIP (128-row)", 192, 40, 0),
    _rs("H192-alias", "skip_out aliases skip_in", 192, 40, 0, alias=True),
    _rs("H192-last", "last, H = 192 with x_out == NULL; mode 15: RESSKIP_LAST (64-row)", 192, 40, 1, xout_null=True),
    _rs("H192-last-alias", "last, skip_out aliases skip_in, no x_in", 192, 40, 1, alias=True, xout_null=True),
    _rs("H20-last-noskip", "last with skip_in == NULL", 20, 40, 1, skip_null=True, xout_null=True),
]
EXPECT_RESSKIP = {"H20", "H96", "H192", "last0", "last1", "skip-null", "alias", "xout-null", "generic:T%4", "pipe",
                  "split:RESSKIP/128", "split:RESSKIP_LAST/64", "split:none"}


def _rs_mirror(c):
    M = c.H if c.last else 2 * c.H
    big = M % 128 == 0 or M > 192                                                         # rows_big
    pipe_ok = c.T % 4 == 0
    split = None                                                                          # conv_split_has
    if pipe_ok and c.last and not big:
        split = "RESSKIP_LAST/64"
    elif pipe_ok and not c.last and big:
        split = "RESSKIP/128"
    L = {f"H{c.H}", f"last{c.last}", "pipe" if pipe_ok else "generic:T%4", "split:" + (split or "none")}
    L |= {"skip-null"} if c.skip_null else set()
    L |= {"alias"} if c.alias else set()
    L |= {"xout-null"} if c.xout_null else set()
    return types.SimpleNamespace(split=split, labels=L)


@functools.lru_cache(maxsize=None)
def _rs_inputs(name, kind):
    c = next(c for c in RESSKIP if c.name == name)
    gen = _gen(c.H, c.T, c.last, len(kind), len(name))
    r = (lambda *s: _ints(gen, *s)) if kind == "count" else (lambda *s: _randn(gen, *s))
    M = c.H if c.last else 2 * c.H
    I = types.SimpleNamespace(kind=kind)
    I.lengths = _ragged(gen, c.B, c.T)
    I.mask = _mask(I.lengths, c.T)
    I.acts = r(c.B, c.H, c.T) if kind == "count" else 0.5 * r(c.B, c.H, c.T)
    I.w = _weight(kind, gen, M, c.H, 1)
    I.wp = _pack_f(I.w)
    I.bias = r(M) if kind == "count" else 0.1 * r(M)
    I.x_in, I.skip_in = r(c.B, c.H, c.T), (None if c.skip_null else r(c.B, c.H, c.T))
    return I


def _rs_ref(c, I, dt):
    t = lambda a: None if a is None else a.to(dt)
    H, m = c.H, t(I.mask)[:, None]
    rs = _conv(t(I.acts), t(I.w), 1, 0) + t(I.bias).view(1, -1, 1)
    s = _conv(t(I.acts).abs(), t(I.w).abs(), 1, 0) + t(I.bias).abs().view(1, -1, 1)
    skip = torch.zeros_like(rs[:, :H]) if I.skip_in is None else t(I.skip_in)
    if c.last:
        return {"skip_out": ((skip + rs) * m, (skip.abs() + s) * m, True)}
    return {"x_out": ((t(I.x_in) + rs[:, :H]) * m, (t(I.x_in).abs() + s[:, :H]) * m, True),
            "skip_out": (skip + rs[:, H:], skip.abs() + s[:, H:], False)}


@gpu
@pytest.mark.parametrize("c", _ids(RESSKIP))
def test_conv_res_skip_fwd(G, c):
    """rs = W acts + b; x_out = (x_in + rs[:H]) mask, skip_out = skip_in + rs[H:]; last: skip_out = (skip_in + rs) mask."""
    mir = _rs_mirror(c)
    B, H, T = c.B, c.H, c.T
    for kind in ("count", "random"):
        I = _rs_inputs(c.name, kind)
        want = _rs_ref(c, I, F64)
        if kind == "count":
            _assert_exact(c.name, *[v[1] for v in want.values()])
        got = {}
        for mode in MODES:
            D = _Dev()
            wp_ptr = D.inp("wp", I.wp)
            if c.alias:
                skip_out = skip_in = D.out("skip_out", B * H * T, init=I.skip_in)
            else:
                skip_in, skip_out = D.inp("skip_in", I.skip_in), D.out("skip_out", B * H * T)
            x_in = None if c.last and c.xout_null else D.inp("x_in", I.x_in)
            x_out = None if c.xout_null else D.out("x_out", B * H * T)
            args = [D.inp("acts", I.acts), wp_ptr, D.inp("bias", I.bias), D.inp("mask", I.mask), x_in, skip_in, x_out, skip_out,
                    B, H, T, c.last]
            _set_mode(G, mode, wp_ptr, I.wp.numel())
            G.hip.call("glowtts_conv_res_skip_fwd", *args)
            r = {k: v.reshape(B, H, T) for k, v in D.finish().items()}
            if c.last and "x_out" in r:
                assert bool((r.pop("x_out") == GUARD).all()), "last = 1 leaves x_out untouched"
            got[mode] = r
            assert set(r) == set(want)
            figs = []
            for name, (value, scale, masked) in want.items():
                _check_elem(f"conv_res_skip_fwd {c.name} {kind} mode {mode}", name, "rs", r[name], value, scale, kind, mode, figs,
                            (I.mask == 0)[:, None] if masked else None)
            print(f"conv_res_skip_fwd {c.name} {kind} mode {mode} [{' '.join(sorted(mir.labels))}]: " + "; ".join(figs))
        same = all(_bits_equal(got[0][n], got[15][n]) for n in got[0])
        if mir.split is None:
            assert same, f"{c.name}: no bf16-plane kernel for this shape, yet mode 15 differs from native"
        elif kind == "random":
            assert not same, f"{c.name}: the mirror expects the bf16-plane kernel {mir.split}, the result is native"


# =============================================================================================== 4. gate backward
def _gb(name, why, H, T, last=False, B=2, drop=False, two=False):
    return _case(name, why, B=B, H=H, T=T, M_rs=H if last else 2 * H, drop=drop, two=two)


GATEBWD = [
    _gb("H20", "H = 20, M_rs = 2H", 20, 40, B=3),
    _gb("H20-T37", "T % 4 != 0: generic kernel", 20, 37, drop=True, B=3),
    _gb("H20-last", "M_rs = H (last layer)", 20, 40, last=True),
    _gb("H20-drop", "drop", 20, 40, drop=True),
    _gb("H192", "H = 192, M_rs = 384: four chunks", 192, 40),
    _gb("H192-last-drop", "H = 192, M_rs = H, drop", 192, 40, last=True, drop=True),
    _gb("H96-two", "two sources at H = 96: one chunk each", 96, 40, two=True),
    _gb("H192-two", "two sources at H = 192: two chunks each, drop", 192, 40, two=True, drop=True),
]
EXPECT_GATEBWD = {"H20", "H96", "H192", "M_rs=2H", "M_rs=H", "drop", "two-source", "generic:T%4", "pipe", "split:GATEBWD/64", "split:none"}


def _gb_mirror(c):
    big = c.H % 128 == 0 or c.H > 192                                                     # rows_big (M = H)
    pipe_ok = c.T % 4 == 0
    split = "GATEBWD/64" if pipe_ok and not big else None                                 # conv_split_has
    L = {f"H{c.H}", "M_rs=2H" if c.M_rs == 2 * c.H else "M_rs=H", "pipe" if pipe_ok else "generic:T%4", "split:" + (split or "none")}
    L |= {"drop"} if c.drop else set()
    L |= {"two-source"} if c.two else set()
    return types.SimpleNamespace(split=split, labels=L)


@functools.lru_cache(maxsize=None)
def _gb_inputs(name, kind):
    c = next(c for c in GATEBWD if c.name == name)
    gen = _gen(c.H, c.T, c.M_rs, len(kind), len(name))
    I = types.SimpleNamespace(kind=kind)
    I.w = _weight(kind, gen, c.M_rs, c.H, 1)              # the res/skip convolution H -> M_rs; the kernel gets its wp_b
    I.wp = _pack_b(I.w)
    if kind == "count":
        I.d = _ints(gen, c.B, c.M_rs, c.T)
        th = torch.randint(-1, 2, (c.B, c.H, c.T), generator=gen).float() / 2
        sg = torch.randint(1, 4, (c.B, c.H, c.T), generator=gen).float() / 4
        I.drop_scale = 2.0
    else:
        I.d = _randn(gen, c.B, c.M_rs, c.T)
        th, sg = torch.tanh(_randn(gen, c.B, c.H, c.T)), torch.sigmoid(_randn(gen, c.B, c.H, c.T))
        I.drop_scale = 1.0 / 0.7
    I.ts = torch.cat([th, sg], 1)
    I.drop = (torch.rand(c.B, 2 * c.H, c.T, generator=gen) < 0.7).to(torch.uint8) if c.drop else None
    return I


def _gb_ref(c, I, dt):
    t = lambda a: a.to(dt)
    H = c.H
    wt = t(I.w).transpose(0, 1).contiguous()             # (H, M_rs, 1): dacts = W^T d_rs
    da, sa = _conv(t(I.d), wt, 1, 0), _conv(t(I.d).abs(), wt.abs(), 1, 0)
    th, sg = t(I.ts[:, :H]), t(I.ts[:, H:])
    ft, fs = sg * (1 - th * th), th * sg * (1 - sg)
    # magnitudes: 1 - th^2 and 1 - sg are differences of 1 and a value below 1: their operands are 1 + th^2 and 1 + sg
    v, s = torch.cat([da * ft, da * fs], 1), torch.cat([sa * sg * (1 + th * th), sa * th.abs() * sg * (1 + sg)], 1)
    if c.drop:
        keep = I.drop.bool()
        v, s = torch.where(keep, v * I.drop_scale, torch.zeros_like(v)), torch.where(keep, s * I.drop_scale, torch.zeros_like(s))
    return v, s


@gpu
@pytest.mark.parametrize("c", _ids(GATEBWD))
def test_conv_gate_bwd(G, c):
    """d_pre = gate'(stored tanh, sigmoid) (W_rs^T d_rs), through the forward's dropout; d_rs in one piece or as two (B, H, T) halves."""
    mir = _gb_mirror(c)
    B, H, T = c.B, c.H, c.T
    for kind in ("count", "random"):
        I = _gb_inputs(c.name, kind)
        want, scale = _gb_ref(c, I, F64)
        if kind == "count":
            _assert_exact(c.name, 16 * scale)             # sixteenths: th^2, sg (1 - sg) are multiples of 1/16 at most
        got = {}
        for mode in MODES:
            D = _Dev()
            wp_ptr = D.inp("wp", I.wp)
            if c.two:
                d1, d2 = D.inp("d_rs", I.d[:, :H]), D.inp("d_rs2", I.d[:, H:])
            else:
                d1, d2 = D.inp("d_rs", I.d), None
            args = [d1, d2, wp_ptr, D.inp("ts", I.ts), D.inp("drop", I.drop), I.drop_scale, D.out("d_pre", B * 2 * H * T), B, c.M_rs, H, T]
            _set_mode(G, mode, wp_ptr, I.wp.numel())
            G.hip.call("glowtts_conv_gate_bwd", *args)
            got[mode] = D.finish()["d_pre"].reshape(B, 2 * H, T)
            figs = []
            _check_elem(f"conv_gate_bwd {c.name} {kind} mode {mode}", "d_pre", "dpre", got[mode], want, scale, kind, mode, figs)
            print(f"conv_gate_bwd {c.name} {kind} mode {mode} [{' '.join(sorted(mir.labels))}]: " + "; ".join(figs))
        if mir.split is None:
            assert _bits_equal(got[0], got[15]), f"{c.name}: no bf16-plane kernel for this shape, yet mode 15 differs from native"
        elif kind == "random":
            assert not _bits_equal(got[0], got[15]), f"{c.name}: the mirror expects the bf16-plane kernel, the result is native"


# =============================================================================================== 5. weight gradients
def _wr(name, why, B, Cin, M, T, taps, dil=1, pad=None, mask=False, mask_x=False, dbias=True, x_slice=False, d_slice=False,
        d_split=0, running=False):
    return _case(name, why, B=B, Cin=Cin, M=M, T=T, taps=taps, dil=dil, pad=(taps - 1) * dil // 2 if pad is None else pad, mask=mask,
                 mask_x=mask_x, dbias=dbias, x_slice=x_slice, d_slice=d_slice, d_split=d_split, running=running)


WRW = [
    # the generic kernel
    _wr("g-T37", "T % 4 != 0: generic kernel, dbias through rowsum; both masks; accumulated from a running sum too", 3, 20, 36, 37, 3,
        mask=True, mask_x=True, running=True),
    _wr("g-nodb", "generic kernel, dbias == NULL, 2 taps with pad 0", 3, 20, 36, 37, 2, pad=0, dbias=False),
    _wr("g-9taps", "9 taps, 162 tiles: 5 splits of B = 7 -> 2 utterances per workgroup, the last has one", 7, 330, 300, 12, 9),
    # convwrw_pipe_kernel: dilation != 1 or a pad other than 'same'
    _wr("p1-40", "1 tap at dilation 2 (no frame-packed form): convwrw_pipe_kernel<1, 40>", 3, 20, 36, 40, 1, dil=2, pad=0, mask=True),
    _wr("p1-32", "convwrw_pipe_kernel<1, 32> (T % 40 != 0), two chunks, the last partial", 3, 20, 36, 36, 1, dil=2, pad=0),
    _wr("p3-40", "convwrw_pipe_kernel<3, 40> at dilation 2, mask_x only", 3, 20, 36, 40, 3, dil=2, mask_x=True),
    _wr("p3-32", "convwrw_pipe_kernel<3, 32>, 3 taps with pad 0 (not 'same'), dbias == NULL", 3, 70, 100, 36, 3, pad=0, dbias=False),
    _wr("p5-40", "convwrw_pipe_kernel<5, 40> at dilation 3 (halo 12), both masks, running sum", 3, 20, 36, 80, 5, dil=3, mask=True,
        mask_x=True, running=True),
    _wr("p5-32", "convwrw_pipe_kernel<5, 32> at dilation 2; x and d channel slices", 3, 20, 36, 36, 5, dil=2, x_slice=True, d_slice=True),
    # the frame-packed kernel: dilation 1, 'same' padding
    _wr("f1-64", "1 tap, 64-frame chunk; mode 15: the split 1-tap kernel with M = 36", 3, 20, 36, 36, 1, mask=True, running=True),
    _wr("f1-80", "1 tap, 80-frame chunks, Cin and M past one 64-tile", 3, 70, 100, 80, 1, mask_x=True),
    _wr("f3-64", "3 taps, 64-frame chunks; mode 15: M = 36 stays native", 3, 20, 36, 100, 3, mask=True, mask_x=True),
    _wr("f3-80", "3 taps, 80-frame chunk; mode 15: transposed-read kernel at 3 taps (M = 32)", 3, 70, 32, 80, 3, mask=True),
    _wr("f5-mt4", "5 taps, M = 36: MT = 4; mode 15: falls back to the native kernel", 3, 20, 36, 36, 5, mask=True, mask_x=True),
    _wr("f5-mt2", "5 taps, M = 32: MT = 2, 80-frame chunk; slices; mode 15: transposed-read, 64 x 32 tiles", 3, 70, 32, 80, 5,
        x_slice=True, d_slice=True, dbias=False),
    _wr("f5-M96", "5 taps, M = 96; mode 15: transposed-read kernel, 64 x 32 tiles (M % 64 != 0)", 3, 70, 96, 64, 5, mask=True),
    _wr("f5-M64", "5 taps, M = 64; mode 15: transposed-read kernel, 64 x 64 tiles", 3, 70, 64, 64, 5, mask_x=True, running=True),
    _wr("f5-span", "5 taps, 48 tiles of 64 x 32: 16 splits of 21 chunks -> 2 chunks per workgroup: a range spans two utterances "
        "(3 chunks each) and the last range holds one chunk", 7, 256, 384, 192, 5, mask=True),
]
WRW2 = [
    _wr("w2-1", "two sources, 1 tap, d_split = 64 of M = 100", 3, 70, 100, 36, 1, d_split=64, running=True),
    _wr("w2-5", "two sources, 5 taps, d_split = 128 of M = 192 (MT = 2); mode 15: transposed-read 64 x 64", 3, 70, 192, 80, 5, d_split=128),
    _wr("w2-5-nodb", "two sources, 5 taps, d_split = 64 of M = 100 (MT = 4), dbias == NULL", 3, 20, 100, 36, 5, d_split=64, dbias=False),
    _wr("w2-3", "two sources, 3 taps, d_split = 64 of M = 96; mode 15: transposed-read at 3 taps", 3, 20, 96, 40, 3, d_split=64),
]
EXPECT_WRW = {"generic", "generic:B-not-multiple-of-split", "generic:rowsum", "pipe<1,40>", "pipe<1,32>", "pipe<3,40>", "pipe<3,32>",
              "pipe<5,40>", "pipe<5,32>", "pad-not-same", "fp<1,64>", "fp<1,80>", "fp<3,64>", "fp<3,80>", "fp<5,64,MT4>", "fp<5,80,MT2>",
              "fp<5,64,MT2>", "partial-tiles", "spans-utterances+short-last", "mask", "mask_x", "mask+mask_x", "x-slice", "d-slice",
              "dbias", "dbias-null", "tr<5,64x64>", "tr<5,64x32>", "tr<3>", "split<1>", "mode15:native"}
EXPECT_WRW2 = {"d_split64", "d_split128", "fp<1,64>", "fp<5,80,MT2>", "fp<5,64,MT4>", "fp<3,64>", "dbias", "dbias-null",
               "tr<5,64x64>", "tr<3>", "split<1>", "mode15:native", "partial-tiles"}


def _wrw_mirror(c):
    """plan_conv_wrw (csrc/convgemm.hip) for glowtts_conv_wrw / _wrw2 with the rules of csrc/conv_plan.hpp and plan_wrw_tr
    (csrc/convwrw_tr.hip) at the default switches."""
    halo, L, geo = (c.taps - 1) * c.dil, set(), None
    pipe_ok = c.T % 4 == 0 and halo <= 12                                                 # wrw_pipe_ok (all tensors aligned here)
    m15 = "native"
    if pipe_ok and c.taps in (1, 3, 5):
        if c.dil == 1 and c.pad == (c.taps - 1) // 2:                                     # wrw_frame_packed
            n5 = c.T % 80 == 0 or -(-c.T // 80) * 80 <= -(-c.T // 64) * 64               # frames80_wrw
            ct = 80 if n5 else 64
            mt = 2 if c.taps == 5 and c.M % 32 == 0 and (not c.d_split or c.d_split % 32 == 0) else 4     # wrw_fp_mt
            L.add(f"fp<{c.taps},{ct}" + (f",MT{mt}>" if c.taps == 5 else ">"))
            tiles, total = -(-c.Cin // 64) * -(-c.M // (16 * mt)), c.B * -(-c.T // ct)   # wrw_split_k
            splits = max(1, min((768 if mt <= 2 else 512) // tiles, total))
            nb, nct = -(-total // splits), -(-c.T // ct)
            geo = (tiles, 1, -(-total // nb), nb)
            spans = any(s // nct != (min(total, s + nb) - 1) // nct for s in range(0, total, nb))
            if spans and total % nb:
                L.add("spans-utterances+short-last")
            if c.M % 32 == 0 and (not c.d_split or c.d_split % 32 == 0) and c.taps == 3:  # plan_wrw_tr
                m15 = "tr<3>"
            elif c.M % 32 == 0 and (not c.d_split or c.d_split % 32 == 0) and c.taps == 5:    # plan_wrw_tr
                m15 = "tr<5,64x64>" if c.M % 64 == 0 and (not c.d_split or c.d_split % 64 == 0) else "tr<5,64x32>"
            elif c.taps == 1:                                                             # plan_conv_wrw: WRW_SPLIT
                m15 = "split<1>"
        else:
            L.add(f"pipe<{c.taps},{40 if c.T % 40 == 0 else 32}>")                        # plan_conv_wrw: WRW_PIPE
            if c.dil == 1:
                L.add("pad-not-same")
    else:
        tiles = -(-c.Cin // 64) * -(-c.M // 128) * c.taps                                 # plan_conv_wrw: WRW_GENERIC
        splits = max(1, min(-(-768 // tiles), c.B))
        nb = -(-c.B // splits)
        geo = (tiles // c.taps, c.taps, -(-c.B // nb), nb)
        L.add("generic")
        if c.B % nb:
            L.add("generic:B-not-multiple-of-split")
        if c.dbias:
            L.add("generic:rowsum")
    L.add("mode15:native" if m15 == "native" else m15)
    if c.Cin % 64 and c.M % 64 and c.Cin > 64 and c.M > 64:
        L.add("partial-tiles")
    L |= {"mask+mask_x"} if c.mask and c.mask_x else {"mask"} if c.mask else {"mask_x"} if c.mask_x else set()
    L |= {"x-slice"} if c.x_slice else set()
    L |= {"d-slice"} if c.d_slice else set()
    L.add("dbias" if c.dbias else "dbias-null")
    L |= {f"d_split{c.d_split}"} if c.d_split else set()
    return types.SimpleNamespace(labels=L, m15=m15, geo=geo)


@functools.lru_cache(maxsize=None)
def _wrw_inputs(name, kind):
    c = next(c for c in WRW + WRW2 if c.name == name)
    gen = _gen(c.B, c.Cin, c.M, c.T, c.taps, len(kind), len(name))
    r = (lambda *s: _ints(gen, *s)) if kind == "count" else (lambda *s: _randn(gen, *s))
    I = types.SimpleNamespace(kind=kind)
    I.lengths = _ragged(gen, c.B, c.T)
    I.mask = _mask(I.lengths, c.T)
    I.x, I.d = r(c.B, c.Cin, c.T), r(c.B, c.M, c.T)
    return I


def _wrw_ref(c, I, dt):
    """dwp[tap][k][m] = sum_{b,t} x[b][k][t + tap dil - pad] d[b][m][t] and dbias[m] = sum_{b,t} d[b][m][t] (masked), with the sums
    of the absolute terms."""
    x, d, m = I.x.to(dt), I.d.to(dt), I.mask.to(dt)[:, None]
    x, d = (x * m if c.mask_x else x), (d * m if c.mask else d)
    halo = (c.taps - 1) * c.dil
    xp = F.pad(x, (c.pad, max(halo - c.pad, 0)))
    sh = [xp[..., tap * c.dil: tap * c.dil + c.T] for tap in range(c.taps)]
    dwp = torch.stack([torch.einsum("bkt,bmt->km", s, d) for s in sh])
    terms = torch.stack([torch.einsum("bkt,bmt->km", s.abs(), d.abs()) for s in sh])
    return {"dwp": (dwp, terms), "dbias": (d.sum((0, 2)), d.abs().sum((0, 2)))}


def _wrw_run(G, c, two):
    mir = _wrw_mirror(c)
    B, Cin, M, T = c.B, c.Cin, c.M, c.T
    for kind in ("count", "random"):
        I = _wrw_inputs(c.name, kind)
        want = _wrw_ref(c, I, F64)
        if not c.dbias:
            want.pop("dbias")
        empty = I.lengths == 0
        if c.mask and c.mask_x and bool(empty.any()):      # the empty row contributes nothing: the same sums without it
            J = types.SimpleNamespace(x=I.x[~empty], d=I.d[~empty], mask=I.mask[~empty])
            for k, (v, _t) in _wrw_ref(c, J, F64).items():
                assert k not in want or torch.equal(v, want[k][0])
        starts = [None] + ([True] if c.running else [])
        for mode in MODES:
            for st in starts:
                gen = _gen(B, Cin, M, T, 5)
                D = _Dev()
                if c.x_slice:
                    x_bs, x_ptr = 2 * Cin * T, D.inp("x", torch.cat([_randn(gen, B, Cin, T), I.x], 1)) + 4 * Cin * T
                else:
                    x_bs, x_ptr = Cin * T, D.inp("x", I.x)
                init = {"dwp": _start(c.taps * Cin * M, 1) if st else 0.0, "dbias": _start(M, 2) if st else 0.0}
                dwp, dbias = D.out("dwp", c.taps * Cin * M, init["dwp"]), (D.out("dbias", M, init["dbias"]) if c.dbias else None)
                _set_mode(G, mode)
                if two:
                    S = c.d_split
                    G.hip.call("glowtts_conv_wrw2", x_ptr, x_bs, D.inp("d", I.d[:, :S]), S * T, D.inp("d2", I.d[:, S:]), (M - S) * T, S,
                               dwp, dbias, B, Cin, M, T, c.taps, c.dil, c.pad)
                else:
                    if c.d_slice:
                        d_bs, d_ptr = 2 * M * T, D.inp("d", torch.cat([I.d, _randn(gen, B, M, T)], 1))
                    else:
                        d_bs, d_ptr = M * T, D.inp("d", I.d)
                    G.hip.call("glowtts_conv_wrw", x_ptr, x_bs, d_ptr, d_bs, D.inp("mask", I.mask) if c.mask else None,
                               D.inp("mask_x", I.mask) if c.mask_x else None, dwp, dbias, B, Cin, M, T, c.taps, c.dil, c.pad)
                r = D.finish()
                figs = []
                for name, (value, terms) in want.items():
                    s0 = init[name].double().reshape(value.shape) if st else torch.zeros_like(value)
                    if kind == "count":
                        _assert_exact(c.name, terms + s0)
                    _check_red(f"conv_wrw {c.name} {kind} mode {mode}", name, r[name].reshape(value.shape), value + s0, terms + s0, kind, figs)
                print(f"conv_wrw {c.name} {kind} mode {mode} start {'sum' if st else '0'} [{' '.join(sorted(mir.labels))}]: " + "; ".join(figs))


@gpu
@pytest.mark.parametrize("c", _ids(WRW))
def test_conv_wrw(G, c):
    """glowtts_conv_wrw: dwp and dbias are ACCUMULATED (from 0, and from a running sum where the row says so)."""
    _wrw_run(G, c, two=False)


@gpu
@pytest.mark.parametrize("c", _ids(WRW2))
def test_conv_wrw2(G, c):
    """glowtts_conv_wrw2: rows [0, d_split) of the output gradient from d, the rest from d2."""
    _wrw_run(G, c, two=True)


# =============================================================================================== 6. rowsum
ROWSUM = [_case("M1", "M = 1: 1024 slabs wanted, B given", B=3, M=1, T=37, mask=True, d_slice=False),
          _case("M1030", "M > 1024: one slab of all utterances", B=3, M=1030, T=5, mask=True, d_slice=False),
          _case("M36-nomask", "no mask, T > 256: the thread loop wraps", B=3, M=36, T=300, mask=False, d_slice=False),
          _case("M36-slice", "d is the lower half of a (B, 2M, T) tensor", B=2, M=36, T=40, mask=True, d_slice=True)]


@gpu
@pytest.mark.parametrize("c", _ids(ROWSUM))
def test_rowsum(G, c):
    """out[m] += sum_{b,t} d[b][m][t] (mask): from 0 and from a running sum."""
    for kind in ("count", "random"):
        gen = _gen(c.B, c.M, c.T, len(kind))
        d = _ints(gen, c.B, c.M, c.T) if kind == "count" else _randn(gen, c.B, c.M, c.T)
        mask = _mask(_ragged(gen, c.B, c.T), c.T)
        dm = d.double() * mask.double()[:, None] if c.mask else d.double()
        want, terms = dm.sum((0, 2)), dm.abs().sum((0, 2))
        for st in (None, _start(c.M, 3)):
            D = _Dev()
            d_ptr = D.inp("d", torch.cat([d, _randn(gen, c.B, c.M, c.T)], 1) if c.d_slice else d)
            out = D.out("out", c.M, 0.0 if st is None else st)
            G.hip.call("glowtts_rowsum", d_ptr, (2 if c.d_slice else 1) * c.M * c.T, D.inp("mask", mask) if c.mask else None, out, c.B, c.M, c.T)
            s0 = torch.zeros(c.M, dtype=F64) if st is None else st.double()
            figs = []
            _check_red(f"rowsum {c.name} {kind}", "out", D.finish()["out"], want + s0, terms + s0, kind, figs)
            print(f"rowsum {c.name} {kind} start {'0' if st is None else 'sum'}: " + "; ".join(figs))


# =============================================================================================== 7. pack / un-pack
PACK = [(36, 20, 3, "partial groups both ways"), (16, 32, 1, "whole groups, 1 tap"), (5, 100, 5, "Cout < 16; 500 values per row: the thread loop wraps"),
        (130, 7, 2, "Cin < 16, 9 output groups, even tap count"), (3, 384, 9, "3456 values per row: un-packing without the register copy")]


def _pack_inputs(kind, cout, cin, taps):
    gen = _gen(cout, cin, taps, len(kind))
    if kind == "count":
        return _ints(gen, cout, cin, taps), None
    return _randn(gen, cout, cin, taps) * (cin * taps) ** -0.5, 0.5 + torch.rand(cout, generator=gen)


def _pack_ref(v, g, dt):
    v = v.to(dt)
    if g is None:
        return v, None
    inv = 1.0 / v.reshape(v.shape[0], -1).norm(dim=1)
    return v * (g.to(dt) * inv).view(-1, 1, 1), inv


@gpu
@pytest.mark.parametrize("cout,cin,taps,why", PACK, ids=[f"{a}x{b}x{c}" for a, b, c, _ in PACK])
def test_pack_weight(G, cout, cin, taps, why):
    """wp_f, wp_b (both, or one alone) and 1 / ||v|| against the builders the convolution tests use.  The k slots beyond the channel
    count belong to the caller, who zero-fills them (include/glowtts_hip.h): they must still be exactly 0 afterwards."""
    for kind in ("count", "random"):
        v, g = _pack_inputs(kind, cout, cin, taps)
        w64, inv64 = _pack_ref(v, g, F64)
        for want_f, want_b in ((True, True), (True, False), (False, True)):
            D = _Dev()
            nf, nb = taps * -(-cin // 16) * cout * 16, taps * -(-cout // 16) * cin * 16
            G.hip.call("glowtts_pack_weight", D.inp("v", v), D.inp("g", g), D.out("wp_f", nf, 0.0) if want_f else None,
                       D.out("wp_b", nb, 0.0) if want_b else None, D.out("inv_norm", cout) if g is not None else None, cout, cin, taps)
            r = D.finish()
            figs = []
            for name, build in (("wp_f", _pack_f), ("wp_b", _pack_b)):
                if name not in r:
                    continue
                want, live = build(w64).reshape(-1), build(torch.ones_like(w64)).reshape(-1) != 0
                assert bool((r[name][~live] == 0).all()), f"pack_weight {name}: a slot beyond the channel count is not 0"
                _check_elem(f"pack_weight {kind}", name, "copy" if g is None else "w", r[name], want, want.abs(), kind if g is None else "random", 0, figs)
            if g is not None:
                _check_elem(f"pack_weight {kind}", "inv_norm", "inv", r["inv_norm"], inv64, inv64.abs(), "random", 0, figs)
            print(f"pack_weight {cout}x{cin}x{taps} {kind} f={int(want_f)} b={int(want_b)}: " + "; ".join(figs))


def _unpack_ref(dwp, v, g, dt):
    """(dv, dg) and the sums of their absolute terms: autograd through w = g v / ||v|| of sum(w dW), dW[o][c][tap] = dwp[tap][c][o]."""
    dw, v = dwp.to(dt).permute(2, 1, 0), v.to(dt)
    if g is None:
        return {"dv": (dw, dw.abs())}
    vr, gr = v.clone().requires_grad_(True), g.to(dt).clone().requires_grad_(True)
    norm = vr.reshape(v.shape[0], -1).norm(dim=1)
    ((gr / norm).view(-1, 1, 1) * vr * dw).sum().backward()
    inv = (1.0 / norm.detach()).view(-1, 1, 1)
    dot_abs = (dw * v).abs().sum((1, 2), keepdim=True)
    gn = (g.to(dt).view(-1, 1, 1) * inv).abs()
    return {"dv": (vr.grad, gn * (dw.abs() + v.abs() * dot_abs * inv * inv)), "dg": (gr.grad, (dot_abs * inv).reshape(-1))}


@gpu
@pytest.mark.parametrize("cout,cin,taps,why", PACK, ids=[f"{a}x{b}x{c}" for a, b, c, _ in PACK])
def test_unpack_weight_grad(G, cout, cin, taps, why):
    """dv and dg are ADDED to what is there (0, and at the first shape a running sum); counting inputs without g: dv += dW exactly."""
    for kind in ("count", "random"):
        v, g = _pack_inputs(kind, cout, cin, taps)
        gen = _gen(cout, cin, taps, 11)
        dwp = _ints(gen, taps, cin, cout) if kind == "count" else _randn(gen, taps, cin, cout)
        want = _unpack_ref(dwp, v, g, F64)
        inv = None if g is None else _pack_ref(v, g, F64)[1].float()
        for st in [None] + ([True] if (cout, cin, taps) == PACK[0][:3] else []):
            D = _Dev()
            init = {"dv": _start(cout * cin * taps, 4) if st else 0.0, "dg": _start(cout, 5) if st else 0.0}
            G.hip.call("glowtts_unpack_weight_grad", D.inp("dwp", dwp), D.inp("v", v), D.inp("g", g), D.inp("inv_norm", inv),
                       D.out("dv", cout * cin * taps, init["dv"]), D.out("dg", cout, init["dg"]) if g is not None else None, cout, cin, taps)
            r = D.finish()
            figs = []
            for name, (value, terms) in want.items():
                s0 = init[name].double().reshape(value.shape) if st else torch.zeros_like(value)
                _check_red(f"unpack_weight_grad {kind}", name, r[name].reshape(value.shape), value.detach() + s0, terms.detach() + s0, kind, figs)
            print(f"unpack_weight_grad {cout}x{cin}x{taps} {kind} start {'sum' if st else '0'}: " + "; ".join(figs))


# =============================================================================================== 8. degenerate sizes, rejected arguments
def _tiny(D, B, T, wp_off=0, mask=True):
    """The arguments of every entry point at Cin = M = H = 4 (buffers of at least one row, so every pointer is valid)."""
    n = max(B, 1) * 128 * max(T, 1)
    a = types.SimpleNamespace(B=B, T=T)
    a.x, a.d, a.ts = D.inp("x", torch.ones(n)), D.inp("d", torch.ones(n)), D.inp("ts", torch.full((n,), 0.5))
    a.wp = D.inp("wp", torch.ones(16 * 8 * 5), off=wp_off)
    a.bias, a.mask = D.inp("bias", torch.ones(8)), (D.inp("mask", torch.ones(max(B, 1) * max(T, 1))) if mask else None)
    a.y, a.y2, a.dwp, a.dbias = D.out("y", n), D.out("y2", n), D.out("dwp", 5 * 8 * 128), D.out("dbias", 128)
    return a


def _entry_calls(a, H=4, d_split=64, M2=128):
    B, T = a.B, a.T
    return {
        "glowtts_conv_fwd": (a.x, 4 * T, a.wp, a.bias, a.mask, None, 0, a.y, 4 * T, B, 4, 4, T, 3, 1, 1, 0, 1, 0),
        "glowtts_conv_fwd_act": (a.x, 4 * T, a.wp, a.bias, a.mask, None, 0, a.y, 4 * T, B, 4, 4, T, 3, 1, 1, 0, 1, 0, 1, None, 1.0, None, 1.0),
        "glowtts_conv_gate_fwd": (a.x, a.wp, a.bias, None, None, 1.0, a.y, a.y2, B, H, T, 3, 1, 1),
        "glowtts_conv_res_skip_fwd": (a.x, a.wp, a.bias, a.mask, a.d, None, a.y, a.y2, B, 4, T, 0),
        "glowtts_conv_gate_bwd": (a.d, None, a.wp, a.ts, None, 1.0, a.y, B, 2 * H, H, T),
        "glowtts_conv_wrw": (a.x, 4 * T, a.d, 4 * T, a.mask, None, a.dwp, a.dbias, B, 4, 4, T, 3, 1, 1),
        "glowtts_conv_wrw2": (a.x, 4 * T, a.d, d_split * T, a.ts, (M2 - d_split) * T, d_split, a.dwp, a.dbias, B, 4, M2, T, 1, 1, 0),
        "glowtts_rowsum": (a.d, 4 * T, a.mask, a.dbias, B, 4, T),
    }


def _untouched(D, what):
    torch.cuda.synchronize()
    for name, (buf, _lo, _n) in D.outs.items():
        assert bool((buf.cpu() == GUARD).all()), f"{what}: output {name} touched"


@gpu
@pytest.mark.parametrize("B,T", [(0, 8), (2, 0)], ids=["B0", "T0"])
def test_empty_batch_or_no_frames_is_a_no_op(G, B, T):
    """B = 0 or T = 0: every entry point returns 0 and writes nothing."""
    for mode in MODES:
        _set_mode(G, mode)
        D = _Dev()
        for name, args in _entry_calls(_tiny(D, B, T)).items():
            G.hip.call(name, *args)
        _untouched(D, f"B={B} T={T} mode {mode}")
        D.finish()


@gpu
def test_abi_rejects_before_any_launch(G):
    """Each argument check of the launchers: an error code, glowtts_last_error set, no output touched.  (Every buffer has the full
    size of the call, so nothing could be read or written out of bounds.)"""
    _set_mode(G, 0)

    def rejected(name, match, args, D):
        with pytest.raises(RuntimeError, match=match):
            G.hip.call(name, *args)
        assert re.search(match, G.lib.glowtts_last_error().decode())
        _untouched(D, name)

    D = _Dev()
    calls = _entry_calls(_tiny(D, 2, 8, mask=False))
    for name in ("glowtts_conv_fwd", "glowtts_conv_fwd_act"):
        rejected(name, "mask flag without mask", calls[name], D)
    D = _Dev()
    calls = _entry_calls(_tiny(D, 2, 8), H=2)
    for name in ("glowtts_conv_gate_fwd", "glowtts_conv_gate_bwd"):
        rejected(name, "multiple of 4", calls[name], D)
    D = _Dev()
    rejected("glowtts_conv_wrw2", "d_split", _entry_calls(_tiny(D, 2, 8), d_split=32)["glowtts_conv_wrw2"], D)
    D = _Dev()
    rejected("glowtts_conv_wrw2", "T % 4", _entry_calls(_tiny(D, 2, 6))["glowtts_conv_wrw2"], D)
    D = _Dev()
    calls = _entry_calls(_tiny(D, 2, 8, wp_off=1))
    for name in ("glowtts_conv_fwd", "glowtts_conv_fwd_act", "glowtts_conv_gate_fwd", "glowtts_conv_res_skip_fwd", "glowtts_conv_gate_bwd"):
        rejected(name, "16-byte aligned", calls[name], D)


# =============================================================================================== 9. the tables, on the CPU
def _reached(table, mirror):
    return set().union(*[mirror(c).labels for c in table])


def test_every_branch_is_reached():
    """The labels the mirrors give the rows of each table are exactly the branches the tables are there for."""
    for table, mirror, expect in ((FWD, _fwd_mirror, EXPECT_FWD), (GATE, _gate_mirror, EXPECT_GATE), (RESSKIP, _rs_mirror, EXPECT_RESSKIP),
                                  (GATEBWD, _gb_mirror, EXPECT_GATEBWD), (WRW, _wrw_mirror, EXPECT_WRW), (WRW2, _wrw_mirror, EXPECT_WRW2)):
        got = _reached(table, mirror)
        assert got == expect, (sorted(expect - got), sorted(got - expect))
        assert len({c.name for c in table}) == len(table)
        for c in table:
            assert c.B <= 8 and c.T <= 192 and max(getattr(c, "Cin", 0), getattr(c, "M", 0), 2 * getattr(c, "H", 0)) <= 384, c.name
    span = next(c for c in WRW if c.name == "f5-span")
    assert "spans-utterances+short-last" in _wrw_mirror(span).labels
    assert {(c.M, c.T > 1024 or c.M > 1024) for c in ROWSUM} >= {(1, False), (1030, True)}


# ---- what the library itself says it would launch (glowtts_conv_plan_next): no GPU, dummy addresses --------------------------------
_EPI = {0: "PLAIN", 1: "GATE", 2: "RESSKIP", 3: "RESSKIP_LAST", 4: "ADD", 5: "GATEBWD"}
_WP_FLOATS = 1 << 20          # floats of the dummy packed-weight buffer that the dummy planes are bound to


class _Addr:
    """16-byte aligned integers that stand for device buffers (a planned call looks at their alignment only); mis: 4 bytes off."""

    def __init__(self):
        self.next = 1 << 24

    def __call__(self, mis=False):
        self.next += 1 << 24
        return self.next + (4 if mis else 0)


@pytest.fixture()
def P():
    """The library with the plan constants; restores the arithmetic mode, the plane binding, the arming and every tuning switch."""
    from glow_tts_train import _hip

    lib = _hip.load()
    before = lib.glowtts_conv_math(-1)
    knobs = {}
    ns = types.SimpleNamespace(lib=lib, hip=_hip, knobs=knobs, **{k[len("GLOWTTS_PLAN_"):]: v for k, v in _hip.CONSTANTS.items()
                                                                 if k.startswith("GLOWTTS_PLAN_")})

    def set_knob(name, value):
        if name not in knobs:
            v = ctypes.c_int()
            assert lib.glowtts_get_knob(name.encode(), ctypes.byref(v)) == 0
            knobs[name] = v.value
        assert lib.glowtts_set_knob(name.encode(), value) == 0

    ns.set_knob = set_knob
    yield ns
    for name, value in knobs.items():
        assert lib.glowtts_set_knob(name.encode(), value) == 0
    lib.glowtts_conv_plan_next(None)
    lib.glowtts_conv_bind_planes(None, 0, None)
    assert lib.glowtts_conv_math(before) == 0


def _planned(P, mode, name, *args, wp=None):
    """The plan of the entry point `name` at these arguments in arithmetic `mode` (with dummy planes bound to wp in a plane mode)."""
    lib = P.lib
    assert lib.glowtts_conv_math(mode) == 0
    lib.glowtts_conv_bind_planes(None, 0, None)
    if (mode & 3) and wp is not None:
        assert lib.glowtts_conv_bind_planes(wp, _WP_FLOATS, 1 << 40) == 0
    plan = P.hip.ConvPlan()
    assert lib.glowtts_conv_plan_next(ctypes.byref(plan)) == 0
    rc = getattr(lib, name)(*args, None)
    lib.glowtts_conv_plan_next(None)
    assert rc == 0, (name, lib.glowtts_last_error())
    assert plan.family != P.NONE and plan.launches >= 1 and plan.lds_bytes <= 160 * 1024 and plan.grid_x * plan.grid_y * plan.grid_z >= 1
    return plan


def _fwd_plan(P, c, mode):
    A, B, Cin, M, T = _Addr(), c.B, c.Cin, c.M, c.T
    x_bs = 2 * Cin * T if c.x_slice else Cin * T + (2 if c.x_bs_odd else 0)
    x = A(c.mis == "x") + (4 * Cin * T if c.x_slice else 0)
    a, a_bs = (A(c.mis == "addend"), 2 * M * T if c.a_slice else M * T) if c.addend else (None, 0)
    y_bs = 2 * M * T if c.y_slice else M * T + (2 if c.y_bs_odd else 0)
    y = A(c.mis == "y") + (4 * M * T if c.y_slice else 0)
    wp = A()
    args = [x, x_bs, wp, A(), A() if (c.mask_in or c.mask_out or c.mask_add) else None, a, a_bs, y, y_bs, B, Cin, M, T, c.taps, c.dil, c.pad,
            c.mask_in, c.mask_out, c.mask_add]
    if c.act:
        return _planned(P, mode, "glowtts_conv_fwd_act", *args, c.relu, A() if c.drop else None, 2.0, A() if c.gate_pos else None, 2.0, wp=wp)
    return _planned(P, mode, "glowtts_conv_fwd", *args, wp=wp)


def _gate_plan(P, c, mode):
    A = _Addr()
    wp = A()
    return _planned(P, mode, "glowtts_conv_gate_fwd", A(), wp, A(), A() if c.cond else None, A() if c.drop else None, 2.0, A(),
                    None if c.ts_null else A(), c.B, c.H, c.T, c.taps, c.dil, c.pad, wp=wp)


def _rs_plan(P, c, mode):
    A = _Addr()
    wp = A()
    skip = None if c.skip_null else A()
    return _planned(P, mode, "glowtts_conv_res_skip_fwd", A(), wp, A(), A(), None if c.last and c.xout_null else A(), skip,
                    None if c.xout_null else A(), skip if c.alias else A(), c.B, c.H, c.T, c.last, wp=wp)


def _gb_plan(P, c, mode):
    A = _Addr()
    wp = A()
    return _planned(P, mode, "glowtts_conv_gate_bwd", A(), A() if c.two else None, wp, A(), A() if c.drop else None, 2.0, A(), c.B, c.M_rs,
                    c.H, c.T, wp=wp)


def _wrw_plan(P, c, mode):
    A, B, Cin, M, T = _Addr(), c.B, c.Cin, c.M, c.T
    x, x_bs = A() + (4 * Cin * T if c.x_slice else 0), (2 if c.x_slice else 1) * Cin * T
    dbias = A() if c.dbias else None
    if c.d_split:
        S = c.d_split
        return _planned(P, mode, "glowtts_conv_wrw2", x, x_bs, A(), S * T, A(), (M - S) * T, S, A(), dbias, B, Cin, M, T, c.taps, c.dil, c.pad)
    return _planned(P, mode, "glowtts_conv_wrw", x, x_bs, A(), (2 if c.d_slice else 1) * M * T, A() if c.mask else None,
                    A() if c.mask_x else None, A(), dbias, B, Cin, M, T, c.taps, c.dil, c.pad)


def _wrw_label(P, plan):
    """The label of _wrw_mirror that a weight-gradient plan stands for."""
    if plan.family == P.WRW_GENERIC:
        return "generic"
    if plan.family == P.WRW_PIPE:
        return f"pipe<{plan.taps},{plan.frame_tile}>"
    if plan.family == P.WRW_FP:
        return f"fp<{plan.taps},{plan.frame_tile}" + (f",MT{plan.mt}>" if plan.taps == 5 else ">")
    if plan.family == P.WRW_TR:
        return "tr<3>" if plan.taps == 3 else f"tr<5,64x{16 * plan.mt}>"
    assert plan.family == P.WRW_SPLIT, plan.family
    return f"split<{plan.taps}>"


# Rows at the edges of the rules that the shape tables (B <= 8, T <= 192) cannot reach; planned on the CPU only.  T = 300 and 304 round
# to 320 frames with 80- and with 64-frame tiles: the forward-type rule (frames80_fwd) takes 64 there, the weight-gradient rule
# (frames80_wrw) 80 — as found, and pinned here.  38 x 2 x 5 = 380 tiles of 128 rows x 80 frames is the first grid that keeps its
# 80-frame tiles (fwd_use32: fewer than 380 workgroups take 32-frame tiles).
EDGE_FWD = [_fwd("edge-T300", "T = 300, addend (no 32-frame tiles): 64-frame tiles", 16, 36, 300, 3, addend=True),
            _fwd("edge-T304", "T = 304: the same tie", 16, 36, 304, 3, addend=True),
            _fwd("edge-T320", "T = 320: 80-frame tiles", 16, 36, 320, 3, addend=True),
            _fwd("edge-wg370", "370 tiles of 80 frames: 32-frame tiles", 16, 640, 160, 3, B=37),
            _fwd("edge-wg380", "380 tiles of 80 frames: they stay", 16, 640, 160, 3, B=38)]
EDGE_WRW = [_wr("edge-T300", "T = 300: 80-frame chunks", 3, 20, 36, 300, 1), _wr("edge-T304", "T = 304: 80-frame chunks", 3, 20, 36, 304, 1),
            _wr("edge-T256", "T = 256: 64-frame chunks", 3, 20, 36, 256, 1)]


def _fwd_type_tables():
    """(table, mirror, planner, the mirror's `split` label of a bf16-plane plan) of the four forward-type tables."""
    return ((FWD + EDGE_FWD, _fwd_mirror, _fwd_plan, lambda p: "PLAIN3/32f" if p.frame_tile == 32 else f"{_EPI[p.epi]}{p.taps}/{p.rows}"),
            (GATE, _gate_mirror, _gate_plan, lambda p: f"{_EPI[p.epi]}{p.taps}"),
            (RESSKIP, _rs_mirror, _rs_plan, lambda p: f"{_EPI[p.epi]}/{p.rows}"),
            (GATEBWD, _gb_mirror, _gb_plan, lambda p: f"{_EPI[p.epi]}/{p.rows}"))


def test_plans_agree_with_the_mirrors(P):
    """For every row of FWD, GATE, RESSKIP, GATEBWD, WRW and WRW2, natively and in mode 15, the row's real entry point is asked what it
    would launch (glowtts_conv_plan_next; integer dummy addresses with the row's alignment): family, rows, frame tile, vector
    epilogue, bf16-plane form, weight-gradient form, nb, grid and launch count must be what the mirror derived.  A rule moved in
    csrc/conv_plan.hpp or in a planner without the mirror (or the other way round) fails here, on a named row."""
    for table, mirror, planner, split_label in _fwd_type_tables():
        for c in table:
            mir = mirror(c)
            generic = any(l.startswith("generic:") for l in mir.labels)
            for mode in MODES:
                plan, what = planner(P, c, mode), f"{c.name} mode {mode}"
                if mode == 15 and mir.split is not None:
                    assert (plan.family, plan.ns, plan.nsa, plan.iob) == (P.SPLIT, 3, 3, 0), what
                    assert split_label(plan) == mir.split, (what, split_label(plan), mir.split)
                else:
                    assert plan.family == (P.GENERIC if generic else P.PIPE) and plan.ns == 0, (what, plan.family)
                assert plan.taps == (0 if generic else c.taps if hasattr(c, "taps") else 1), what
                assert (plan.block, plan.grid_z, plan.launches, plan.nbatch) == (256, 1, 1, 0), what
                if mirror is _fwd_mirror:
                    nt = 32 if mir.use32 else 80 if mir.n5 else 64
                    assert plan.epi == (4 if c.addend else 0), what
                    assert (plan.rows, plan.frame_tile, plan.vec_epilogue) == (128 if mir.big else 64, nt, int(mir.vec)), \
                        (what, plan.rows, plan.frame_tile, plan.vec_epilogue)
                    assert {f"rows{plan.rows}", f"nt{plan.frame_tile}"} <= mir.labels, what
                    assert (plan.grid_x, plan.grid_y) == (c.B * -(-c.T // nt), -(-c.M // plan.rows)), what
                    if nt == 80:
                        assert plan.grid_x * plan.grid_y == mir.wg5, what
                    if generic:
                        assert plan.xp_pitch % 32 == 16 and 0 <= plan.xp_pitch - (nt + (c.taps - 1) * c.dil) < 32, what
                else:
                    M = 2 * c.H if table is GATE else (c.H if c.last else 2 * c.H) if table is RESSKIP else c.H
                    rows = 128 if table is GATE or M % 128 == 0 or M > 192 else 64
                    assert plan.epi == {id(GATE): 1, id(GATEBWD): 5}.get(id(table), 3 if getattr(c, "last", 0) else 2), what
                    assert plan.rows == rows and plan.frame_tile == (80 if c.T % 80 == 0 else 64), (what, plan.rows, plan.frame_tile)
                    assert plan.grid_y == (-(-c.H // 64) if table is GATE else -(-M // rows)), what
                    assert plan.vec_epilogue == int(not generic), what
    assert [(c.name, _fwd_mirror(c).use32, _fwd_mirror(c).n5) for c in EDGE_FWD] == [
        ("edge-T300", False, False), ("edge-T304", False, False), ("edge-T320", False, True), ("edge-wg370", True, True), ("edge-wg380", False, True)]
    assert [sorted(l for l in _wrw_mirror(c).labels if l.startswith("fp<")) for c in EDGE_WRW] == [["fp<1,80>"], ["fp<1,80>"], ["fp<1,64>"]]
    for table in (WRW + EDGE_WRW, WRW2):
        for c in table:
            mir = _wrw_mirror(c)
            native = _wrw_plan(P, c, 0)
            label = _wrw_label(P, native)
            assert label in mir.labels and native.ns == 0, (c.name, label, sorted(mir.labels))
            assert native.launches == (2 if "generic:rowsum" in mir.labels else 1), c.name
            if mir.geo is not None:
                assert (native.grid_x, native.grid_y, native.grid_z, native.nb) == mir.geo, (c.name, mir.geo)
            assert native.block == 256 and native.nbatch == 0 and native.rows == 64, c.name
            m15 = _wrw_plan(P, c, 15)
            if mir.m15 == "native":
                assert [getattr(m15, f) for f, _ in m15._fields_] == [getattr(native, f) for f, _ in native._fields_], c.name
            else:
                assert _wrw_label(P, m15) == mir.m15 and m15.ns == 3, (c.name, _wrw_label(P, m15), mir.m15)
                assert m15.block == (512 if m15.family == P.WRW_TR else 256), c.name


# What the tuning switches promise (include/glowtts_hip.h, csrc/conv_plan.hpp, csrc/convwrw_tr.hip) at their non-default values: the
# mirrors model the defaults only.  (switch, value, what a mode-15 weight-gradient plan of a row with the default label `was` becomes.)
_TR = lambda mt, w32, ng=2: ("WRW_TR", mt, w32, ng)
KNOB_EXPECT = [
    ("WRW_TR", 0, {"tr<5,64x64>": ("WRW_SPLIT", 2, 0, 0), "tr<5,64x32>": ("WRW_SPLIT", 2, 0, 0), "tr<3>": ("WRW_FP", 4, 0, 0)}),
    ("WRW_TR", 1, {"tr<5,64x64>": _TR(2, 0), "tr<5,64x32>": _TR(2, 0), "tr<3>": _TR(2, 1)}),
    ("WRW_TR_MT", 2, {"tr<5,64x64>": _TR(2, 1), "tr<5,64x32>": _TR(2, 1), "tr<3>": _TR(2, 1)}),
    ("WRW_TR3", 0, {"tr<5,64x64>": _TR(4, 0), "tr<5,64x32>": _TR(2, 1), "tr<3>": ("WRW_FP", 4, 0, 0)}),
    ("WRW_TR3_MT", 4, {"tr<5,64x64>": _TR(4, 0), "tr<5,64x32>": _TR(2, 1), "tr<3>": _TR(2, 1), "tr<3>/M64": _TR(4, 0)}),
    ("WRW_TR_NG", 1, {"tr<5,64x64>": _TR(4, 0, 1), "tr<5,64x32>": _TR(2, 1), "tr<3>": _TR(2, 1)}),
]
# shapes the tables do not hold: a 3-tap weight gradient with M % 64 == 0 (GLOWTTS_WRW_TR3_MT), and a plain 1x1 convolution whose
# 80-frame grid is past the small-grid rule (480 tiles), so that only GLOWTTS_CONV32_1X1 gives it 32-frame tiles
KNOB_WRW3_M64 = _wr("k-f3-M64", "3 taps, M = 64", 3, 70, 64, 80, 3)
KNOB_1X1 = _fwd("k-1x1", "the coupling's end conv at the benchmark's size", 192, 160, 400, 1, B=32)


def test_plans_follow_the_tuning_switches(P):
    """The rows again with each launch-geometry switch at its non-default value: the default plan first (the mirror's), then the
    family / tile the header promises for the switch.  Every switch is restored afterwards (fixture)."""
    rows = [(c, _wrw_mirror(c).m15) for c in WRW + WRW2] + [(KNOB_WRW3_M64, "tr<3>/M64")]
    assert {m for _, m in rows} >= {"tr<5,64x64>", "tr<5,64x32>", "tr<3>", "tr<3>/M64", "split<1>", "native"}
    default, native = {c.name: _wrw_plan(P, c, 15) for c, _ in rows}, {c.name: _wrw_plan(P, c, 0) for c, _ in rows}
    fields = lambda p: [getattr(p, f) for f, _ in p._fields_]
    for c, was in rows:
        if was.startswith("tr<"):
            want = _TR(2, 1) if was == "tr<3>/M64" else _TR(4, 0) if was == "tr<5,64x64>" else _TR(2, 1)
            p = default[c.name]
            assert ("WRW_TR", p.mt, p.w32, p.ng) == want, (c.name, was)
    for knob, value, expect in KNOB_EXPECT:
        P.set_knob(knob, value)
        for c, was in rows:
            p = _wrw_plan(P, c, 15)
            if was in expect or (was == "tr<3>/M64" and "tr<3>" in expect):
                family, mt, w32, ng = expect.get(was, expect["tr<3>"])
                assert (p.family, p.mt, p.w32, p.ng) == (getattr(P, family), mt, w32, ng), (knob, value, c.name, was, p.family, p.mt, p.w32, p.ng)
                assert p.block == (256 * ng if family == "WRW_TR" else 256), (knob, c.name)
            else:                                          # 1-tap and native rows: these switches are about 5 and 3 taps
                assert fields(p) == fields(default[c.name]), (knob, value, c.name)
            assert fields(_wrw_plan(P, c, 0)) == fields(native[c.name]), (knob, value, c.name)       # fp32 arithmetic: no switch applies
        P.set_knob(knob, P.knobs[knob])
    # GLOWTTS_CONV32_1X1 = 0: plain 1x1 convolutions on 80- / 64-frame tiles — where the small-grid rule does not ask for 32 anyway
    for value, nt in ((1, 32), (0, 80)):
        P.set_knob("CONV32_1X1", value)
        for mode in MODES:
            assert _fwd_plan(P, KNOB_1X1, mode).frame_tile == nt, (value, mode)
        for c in FWD:                                      # the tables' shapes are all below 380 workgroups: the switch changes nothing
            mir = _fwd_mirror(c)
            assert _fwd_plan(P, c, 0).frame_tile == (32 if mir.use32 else 80 if mir.n5 else 64), (value, c.name)


def test_batch_plans_count_their_launches(P):
    """glowtts_conv_wrw_batch: whether a group of up to four problems goes as ONE launch is plan_conv_wrw's answer (only the
    bf16-plane kernels take a batch); the plan of an armed call describes the first launch and counts all of them."""
    def batch(c, n, mode):
        A = _Addr()
        arr = lambda: (ctypes.c_void_p * n)(*[A() for _ in range(n)])
        x, d, dwp, dbias = arr(), arr(), arr(), (arr() if c.dbias else None)
        return _planned(P, mode, "glowtts_conv_wrw_batch", n, x, c.Cin * c.T, d, c.M * c.T, None, 0, 0, A() if c.mask else None,
                        A() if c.mask_x else None, dwp, dbias, c.B, c.Cin, c.M, c.T, c.taps, c.dil, c.pad)

    rows = {c.name: c for c in WRW}
    for name, n, want15 in (("f5-M64", 6, (P.WRW_TR, 4, 2)),        # 5 taps, M % 64 == 0: groups of 4 and 2, one launch each
                            ("f1-64", 5, (P.WRW_SPLIT, 4, 2)),       # the 1-tap bf16-plane kernel takes a batch as well: 4 + 1
                            ("f5-mt4", 6, (P.WRW_FP, 0, 6)),         # M = 36: no plane kernel, so problem by problem in either mode
                            ("g-T37", 3, (P.WRW_GENERIC, 0, 6))):    # generic kernel + row sums: two launches per problem
        c = rows[name]
        one = _wrw_plan(P, c, 0)
        p0 = batch(c, n, 0)
        assert (p0.family, p0.nbatch, p0.launches) == (one.family, 0, n * one.launches), (name, p0.family, p0.nbatch, p0.launches)
        assert (p0.grid_x, p0.grid_y, p0.grid_z, p0.nb) == (one.grid_x, one.grid_y, one.grid_z, one.nb), name
        p15 = batch(c, n, 15)
        assert (p15.family, p15.nbatch, p15.launches) == want15, (name, p15.family, p15.nbatch, p15.launches)
        if p15.nbatch:
            single = _wrw_plan(P, c, 15)
            assert p15.grid_x == single.grid_x and p15.grid_z % p15.nbatch == 0 and p15.lds_bytes == single.lds_bytes, name


@gpu
def test_an_armed_call_launches_nothing(G):
    """glowtts_conv_plan_next on the GPU, at the first FWD and the first WRW row: the armed call returns 0, fills the plan and leaves
    every guarded output buffer at GUARD; the same call again, unarmed, gives the row's result."""
    c, plan = FWD[0], G.hip.ConvPlan()
    I = _fwd_inputs(c.name, "random")
    y = _fwd_launch(G, c, I, 0, arm=plan)
    assert bool((y == GUARD).all()) and plan.family == G.hip.CONSTANTS["GLOWTTS_PLAN_GENERIC"] and plan.launches == 1
    want, scale = _fwd_ref(c, I, F64)
    _check_elem(f"conv_fwd {c.name} after an armed call", "y", "y", _fwd_launch(G, c, I, 0), want, scale, "random", 0, [])

    c = WRW[0]
    I = _wrw_inputs(c.name, "random")
    want = _wrw_ref(c, I, F64)
    for armed in (True, False):
        D = _Dev()
        dwp, dbias = D.out("dwp", c.taps * c.Cin * c.M, None if armed else 0.0), D.out("dbias", c.M, None if armed else 0.0)
        args = [D.inp("x", I.x), c.Cin * c.T, D.inp("d", I.d), c.M * c.T, D.inp("mask", I.mask), D.inp("mask_x", I.mask), dwp, dbias,
                c.B, c.Cin, c.M, c.T, c.taps, c.dil, c.pad]
        _set_mode(G, 0)
        if armed:
            assert G.lib.glowtts_conv_plan_next(ctypes.byref(plan)) == 0
        G.hip.call("glowtts_conv_wrw", *args)
        if armed:
            _untouched(D, "armed glowtts_conv_wrw")
            assert plan.family == G.hip.CONSTANTS["GLOWTTS_PLAN_WRW_GENERIC"] and plan.launches == 2
        r = D.finish()
        if not armed:
            for name, (value, terms) in want.items():
                _check_red(f"conv_wrw {c.name} after an armed call", name, r[name].reshape(value.shape), value, terms, "random", [])


def _fp32_cpu_figures():
    """key -> the worst figure of plain fp32 torch on the CPU against fp64 over the tables (the 'fp32 CPU' column of the module
    docstring), and the worst reduction figure in units of sum|term|."""
    figs, red = {k: 0.0 for k in BOUNDS}, 0.0

    def upd(key, got, want, scale):
        figs[key] = max(figs[key], _units(got, want, scale))

    for c in FWD:
        I = _fwd_inputs(c.name, "random")
        (w64, s), (w32, _) = _fwd_ref(c, I, F64), _fwd_ref(c, I, F32)
        upd("y", w32, w64, s)
    for c in GATE:
        I = _gate_inputs(c.name, "random")
        r64, r32 = _gate_ref(c, I, F64)[0], _gate_ref(c, I, F32)[0]
        for name, (key, value, scale) in r64.items():
            upd(key, r32[name][1], value, scale)
    for c in RESSKIP:
        I = _rs_inputs(c.name, "random")
        r64, r32 = _rs_ref(c, I, F64), _rs_ref(c, I, F32)
        for name, (value, scale, _m) in r64.items():
            upd("rs", r32[name][0], value, scale)
    for c in GATEBWD:
        I = _gb_inputs(c.name, "random")
        (w64, s), (w32, _) = _gb_ref(c, I, F64), _gb_ref(c, I, F32)
        upd("dpre", w32, w64, s)
    for c in WRW + WRW2:
        I = _wrw_inputs(c.name, "random")
        r64, r32 = _wrw_ref(c, I, F64), _wrw_ref(c, I, F32)
        for name, (value, terms) in r64.items():
            red = max(red, _red_fig(r32[name][0], value, terms))
    for cout, cin, taps, _why in PACK:
        v, g = _pack_inputs("random", cout, cin, taps)
        (w64, i64), (w32, i32) = _pack_ref(v, g, F64), _pack_ref(v, g, F32)
        upd("w", w32, w64, w64.abs())
        upd("inv", i32, i64, i64.abs())
        dwp = _randn(_gen(cout, cin, taps, 11), taps, cin, cout)
        r64, r32 = _unpack_ref(dwp, v, g, F64), _unpack_ref(dwp, v, g, F32)
        for name, (value, terms) in r64.items():
            red = max(red, _red_fig(r32[name][0].detach(), value.detach(), terms.detach()))
    return figs, red


def test_bound_table_matches_fp32_cpu_evaluation():
    """Every element-wise bound is 4 x the fp32-CPU figure rounded up to a power of two: fig <= bound <= 16 fig (4 x, the rounding
    to a power of two, and a factor 2 for another CPU's vector width); copies have bound 0 and figure 0."""
    figs, red = _fp32_cpu_figures()
    for key, fig in sorted(figs.items()):
        print(f"fp32 CPU {key}: {fig:.2f} u (bound {BOUNDS[key]}, mode 15: {BOUNDS[key] + SPLIT_EXTRA if BOUNDS[key] else 0})")
    print(f"fp32 CPU reductions: {red:.1e} of sum|term| (the bound 1e-5 is the project's figure for the kernels' reduction "
          "structure, not a measurement)")
    assert red <= 1e-5
    for key, fig in figs.items():
        bound = BOUNDS[key]
        if key == "copy":
            assert fig == 0 and bound == 0
            continue
        assert bound == 2 ** round(math.log2(bound)), key
        assert fig <= bound <= 16 * fig, (key, fig, bound)


def _bf16_planes(x):
    """The three bf16 planes of fp32 values as csrc/split_planes.hpp makes them: round to nearest even, then the exact remainder."""
    planes, rest = [], x.clone()
    for _ in range(3):
        p = rest.to(torch.bfloat16).float()
        planes.append(p)
        rest = rest - p
    return planes, rest


def test_counting_inputs_are_exact_on_the_cpu():
    """The counting inputs give the same result in fp32 and fp64 with plain torch (what the GPU tests assert EQUAL is exact in fp32
    whatever the order of the sums), and in the emulated three-plane split: a small integer (and a counting tanh / sigmoid value)
    is its own plane 0 with planes 1 and 2 zero, so the six products kept are the one exact product."""
    for c in FWD:
        I = _fwd_inputs(c.name, "count")
        (w64, s), (w32, _) = _fwd_ref(c, I, F64), _fwd_ref(c, I, F32)
        _assert_exact(c.name, s)
        assert torch.equal(w32.double(), w64) and bool((w64 == w64.round()).all()), c.name
        for t in (I.x, I.wp, I.bias):
            planes, rest = _bf16_planes(t)
            assert torch.equal(planes[0], t) and not planes[1].any() and not planes[2].any() and not rest.any()
        if c.bwd:      # the packed backward weights ARE the forward packing of the flipped, transposed weights, and the reference
            assert torch.equal(_pack_b(I.w_orig), _pack_f(I.w))                          # is the input gradient of that convolution
            xr = torch.zeros(c.B, c.M, c.T, dtype=F64, requires_grad=True)
            halo = (c.taps - 1) * c.dil
            (_conv(xr, I.w_orig.double(), c.dil, halo - c.pad) * I.x.double()).sum().backward()
            assert torch.equal(xr.grad, _conv(I.x.double(), I.w.double(), c.dil, c.pad)), c.name
    for c in RESSKIP:
        I = _rs_inputs(c.name, "count")
        r64, r32 = _rs_ref(c, I, F64), _rs_ref(c, I, F32)
        for name in r64:
            assert torch.equal(r32[name][0].double(), r64[name][0]), (c.name, name)
    for c in GATEBWD:
        I = _gb_inputs(c.name, "count")
        (w64, s), (w32, _) = _gb_ref(c, I, F64), _gb_ref(c, I, F32)
        _assert_exact(c.name, 16 * s)
        assert torch.equal(w32.double(), w64) and bool((64 * w64 == (64 * w64).round()).all()), c.name
        planes, rest = _bf16_planes(I.ts)
        assert torch.equal(planes[0], I.ts) and not planes[1].any() and not rest.any()
    for c in WRW + WRW2:
        I = _wrw_inputs(c.name, "count")
        r64, r32 = _wrw_ref(c, I, F64), _wrw_ref(c, I, F32)
        for name in r64:
            _assert_exact(c.name, r64[name][1] + 3)
            assert torch.equal(r32[name][0].double(), r64[name][0]), (c.name, name)
    for c in GATE:
        pre64, pre32 = _gate_ref(c, _gate_inputs(c.name, "count"), F64)[1], _gate_ref(c, _gate_inputs(c.name, "count"), F32)[1]
        assert torch.equal(pre32.double(), pre64) and int((pre64[:, :c.H] == 0).sum()) > 0 and int((pre64[:, c.H:] == 0).sum()) > 0, c.name
    # random values: the three planes add up to the value bit for bit, and the products dropped are below 2 u |x w|
    x, w = torch.randn(4096, generator=_gen(1)), torch.randn(4096, generator=_gen(2))
    (px, rx), (pw, rw) = _bf16_planes(x), _bf16_planes(w)
    assert not rx.any() and not rw.any()
    kept = sum(px[i].double() * pw[j].double() for i in range(3) for j in range(3) if i + j <= 2)
    assert bool(((x.double() * w.double() - kept).abs() <= SPLIT_EXTRA * U * (x.double() * w.double()).abs()).all())


def test_python_packing_matches_the_documented_layout():
    """_pack_f / _pack_b against the index formulas of include/glowtts_hip.h, element by element."""
    cout, cin, taps = 19, 21, 3
    w = torch.arange(cout * cin * taps, dtype=F32).reshape(cout, cin, taps) + 1
    pf, pb = _pack_f(w), _pack_b(w)
    assert pf.shape == (taps, 2, cout, 16) and pb.shape == (taps, 2, cin, 16)
    for o in range(cout):
        for k in range(cin):
            for tap in range(taps):
                assert pf[tap, k // 16, o, k % 16] == w[o, k, tap] and pb[taps - 1 - tap, o // 16, k, o % 16] == w[o, k, tap]
    assert int((pf != 0).sum()) == w.numel() == int((pb != 0).sum())
