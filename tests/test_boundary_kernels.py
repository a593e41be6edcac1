"""The three kernels of csrc/flow_boundary.hip one by one, through the C ABI (glow_tts_train._hip.call), against plain fp64 torch
on the CPU: glowtts_flow_boundary_fwd, glowtts_flow_boundary_bwd and glowtts_flow_boundary_bwd_reduce.  The parity tests compare
them with three other kernels of the library that share their formulas, layout and channel map, on inputs that are already
masked; here the reference is written from the header's four lines, index by index, and uses nothing of the package.  The GPU
tests are marked `gpu`; the tests at the end of the module check the bound table and the counting inputs on the CPU.

Every launch (tests/helpers.py: Dev): each input is a copy inside a guarded buffer and must be bit-identical afterwards; each
output lives between guard sentinels that must survive and is pre-filled with the sentinel; the accumulated outputs (logdet_prev,
dlogs, dbias, dw) start from known non-zero values.  Lengths are ragged; from two utterances on, one has length 0; one length ends
inside a frame quad; inputs beyond an utterance's end hold random finite values and are NOT masked.

Forward (include/glowtts_hip.h):   out = W_end skip + b_end
                                   z = [y_prev0 ; (m + e^logs' y_prev1) mask], (m, logs') = out, logdet_prev += sum logs' mask
                                   y = W ((bias + e^logs z) mask) mask over groups of n_split channels,
                                   logdet = (sum logs + logdet_w C / n_split) x_len
                                   h0 = (W_start y[:, :C/2] + b_start) mask
Backward: fp64 autograd over that forward with out_prev a leaf, loss <y, dy_next> + <h0, dx_wn> + <dlogdet, logdet_prev + logdet>;
dskip = W_end^T dout_prev (times the mask when mask_dskip); the parameter gradients are ADDED to their starts.  The partials'
sums are the parameter gradients of the loss without <dlogdet, logdet> (what the reduce entry adds when dlogdet is NULL).

Rows (B, C, H, T, n_split): see ROWS.  Each with sigmoid_scale 0 and 1, the backward with mask_dskip 0 and 1 and, on two rows, with
dlogdet NULL (in both launches).

Random inputs: logs, bias ~ 0.1 N; W = QR factor with det > 0, w_inv / logdet_w from fp64; conv weights ~ 0.7 N / sqrt(fan-in).
Bounds in u = 2**-24 times a scale.  out, h0, dskip: the sum of |terms| of the dot product plus |bias|.  The other element-wise
outputs: the same formulas evaluated on absolute values (every sum a sum of |terms|, an exponential's scale multiplied by
1 + |argument|).  Reductions (logdet_prev, logdet, dlogs, dbias, dw and the partials' sums): the sum of |terms|, |start| included.
Each bound is 4 x what the same formulas in fp32 torch on the CPU show against fp64 on the same inputs (worst over the rows and
variants), rounded up to a power of two; test_bound_table_matches_fp32_cpu_evaluation recomputes the column and asserts
fig <= bound <= 16 fig.
    output        fp32 CPU    bound     MI355X   (dlogs, dbias, dw: the partials' sums included)
    out            4.05 u     32 u    3.46 u
    y              9.03 u     64 u   13.95 u
    h0             5.21 u     32 u    6.08 u
    logdet_prev    2.29 u     16 u    3.24 u
    logdet         1.60 u      8 u    1.60 u
    dy_prev        2.73 u     16 u    3.27 u
    dout_prev      9.79 u     64 u   10.81 u
    dskip          6.18 u     32 u    6.18 u
    dlogs          0.96 u      4 u    1.35 u
    dbias          0.62 u      4 u    0.62 u
    dw             1.92 u      8 u    3.06 u   (the worst of two runs; the reduce adds with atomics)

Counting inputs (sigmoid_scale 0): values and weights are small integers, logs = 0, the logs' rows of the forward's end conv are
zero (e^logs' = 1), logdet_w is handed over as the integer 3 (an independent argument of the ABI), W is a signed permutation with
det +1 that is not symmetric and not its own inverse.  Every sum of |terms| stays below 2**24 (asserted), so every output is exact
in fp32 in any order: out, y, h0, dy_prev, dout_prev and dskip are asserted EQUAL.  A signed permutation is orthogonal, so its
inverse IS its transpose: the counting inputs tell W from W^T = W^-1 (the CPU test shows that every output that reads W changes),
and in the reduce w_inv from w_inv^T.
"""
import functools
import math
import re
import types

import pytest
import torch

from helpers import Dev, GUARD, pack_weight, units

gpu = pytest.mark.gpu

ROWS = [((2, 4, 8, 4, 4), "one group, one quad, H and C/2 far below one k group"),
        ((2, 8, 20, 36, 2), "H leaves the second k group partly empty; last tile of one quad; n_split 2"),
        ((3, 40, 48, 68, 4), "C/2 = 20 leaves the start conv's second k group partly empty; C leaves a row tile partly empty; three "
                             "tiles; one empty utterance; one length of 33 (a mask edge inside a quad at a tile edge)"),
        ((1, 128, 64, 32, 2), "C / n_split = 64, the cap: all 512 items of both passes are live"),
        ((1, 192, 192, 32, 4), "both maxima: 12 row tiles, 12 k groups, 6 start-conv groups")]
ROW_PARAMS = [pytest.param(r, id="x".join(map(str, r))) for r, _why in ROWS]
NULL_DLOGDET_ROWS = (ROWS[1][0], ROWS[2][0])

BOUNDS = {"out": 32, "y": 64, "h0": 32, "logdet_prev": 16, "logdet": 8, "dy_prev": 16, "dout_prev": 64, "dskip": 32, "dlogs": 4,
          "dbias": 4, "dw": 8}          # in u: the table of the module docstring
FWD_OUT = ("out", "y", "h0", "logdet_prev", "logdet")
BWD_OUT = ("dy_prev", "dout_prev", "dskip", "part_dlogs", "part_dbias", "part_dw", "dlogs", "dbias", "dw")
EXACT = ("out", "y", "h0", "dy_prev", "dout_prev", "dskip")


@pytest.fixture(scope="module")
def G():
    from glow_tts_train import _hip

    _hip.load()
    return types.SimpleNamespace(hip=_hip)


# =============================================================================================== inputs
def _signed_perm(n):
    """e_i -> e_{i+1}, e_{n-1} -> -e_0: a cycle with one sign turned, det +1, not symmetric, not its own inverse."""
    w = torch.zeros(n, n)
    for i in range(n - 1):
        w[i + 1, i] = 1.0
    w[0, n - 1] = -1.0
    return w


@functools.lru_cache(maxsize=None)
def _inputs(kind, B, C, H, T, N):
    """Everything the three kernels read, fp32 on the CPU."""
    gen = torch.Generator().manual_seed(7919 * B + 104729 * C + 1299709 * H + 31 * T + N + len(kind))
    I = types.SimpleNamespace(kind=kind, B=B, C=C, H=H, T=T, N=N)
    half = C // 2
    lengths = torch.tensor([T if B >= 3 else T - 1, 0, min(33, T - 1)][:B])   # ragged; one empty; one ends inside a frame quad
    assert B == 1 or int(lengths.min()) == 0
    assert any(int(l) % 4 for l in lengths)
    I.lengths, I.x_len = lengths, lengths.float()
    I.mask = (torch.arange(T)[None] < lengths[:, None]).float()
    rn = lambda *shape: torch.randn(shape, generator=gen)                                   # noqa: E731
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=gen).float()      # noqa: E731
    if kind == "count":
        I.skip, I.y_prev, I.dx_wn, I.dy_next = ri(-2, 2, B, H, T), ri(-2, 2, B, C, T), ri(-2, 2, B, H, T), ri(-2, 2, B, C, T)
        I.W_end_bwd = ri(-1, 1, C, H)
        I.W_end = I.W_end_bwd.clone()
        I.W_end[half:] = 0.0                             # the logs' rows: e^logs' = 1
        I.b_end = ri(-2, 2, C)
        I.b_end[half:] = 0.0
        I.W_start, I.b_start = ri(-1, 1, H, half), ri(-2, 2, H)
        I.logs, I.bias = torch.zeros(C), ri(-2, 2, C)
        I.W = _signed_perm(N)
        I.w_inv, I.logdet_w = I.W.T.contiguous(), torch.tensor([3.0])
        I.out_prev = torch.einsum("ch,bht->bct", I.W_end, I.skip) + I.b_end[None, :, None]   # integers: exact
        I.dlogdet, I.ld0 = ri(-2, 2, B), ri(-3, 3, B)
        I.dlogs0, I.dbias0, I.dw0 = ri(-3, 3, C), ri(-3, 3, C), ri(-3, 3, N, N)
    else:
        I.skip, I.y_prev, I.dx_wn, I.dy_next = rn(B, H, T), rn(B, C, T), rn(B, H, T), rn(B, C, T)
        I.W_end = rn(C, H) * (0.7 / math.sqrt(H))
        I.W_end_bwd = I.W_end
        I.b_end = rn(C) * 0.1
        I.W_start, I.b_start = rn(H, half) * (0.7 / math.sqrt(half)), rn(H) * 0.1
        I.logs, I.bias = rn(C) * 0.1, rn(C) * 0.1
        q = torch.linalg.qr(rn(N, N).double())[0]
        if float(torch.det(q)) < 0:
            q[:, 0] = -q[:, 0]
        I.W = q.float().contiguous()
        I.w_inv = torch.linalg.inv(I.W.double()).float().contiguous()
        I.logdet_w = torch.logdet(I.W.double()).float().reshape(1)
        I.out_prev = rn(B, C, T) * 0.3
        I.dlogdet, I.ld0 = rn(B), rn(B)
        I.dlogs0, I.dbias0, I.dw0 = rn(C), rn(C), rn(N, N)
    return I


# =============================================================================================== the reference
def _grp(x, n):
    """(B, C, T) -> (B, n, C / n, T): the rows an invertible 1x1 convolution mixes (x.view(b, 2, c / n, n / 2, t) with the two
    middle axes swapped): row k of group g is channel (k // (n / 2)) C / 2 + g n / 2 + k % (n / 2)."""
    B, C, T = x.shape
    return x.reshape(B, 2, C // n, n // 2, T).permute(0, 1, 3, 2, 4).reshape(B, n, C // n, T)


def _ungrp(x, n):
    B, _n, g, T = x.shape
    return x.reshape(B, 2, n // 2, g, T).permute(0, 1, 3, 2, 4).reshape(B, n * g, T)


def _flow(P, out, sig, want_scale=False):
    """The header's lines 2 to 4 on tensors of one dtype: (y, h0, logdet_prev, logdet) and, on request, their scales."""
    N, C = P.N, P.C
    half, m3 = C // 2, P.mask[:, None]
    lr = out[:, half:]
    l = torch.log(1e-6 + torch.sigmoid(lr + 2.0)) if sig else lr
    el, e = torch.exp(l), torch.exp(P.logs)[None, :, None]
    z = torch.cat([P.y_prev[:, :half], (out[:, :half] + el * P.y_prev[:, half:]) * m3], 1)
    ld_prev = P.ld0 + (l * m3).sum((1, 2))
    a = (P.bias[None, :, None] + e * z) * m3
    y = _ungrp(torch.einsum("ok,bkgt->bogt", P.W, _grp(a, N)) * P.mask[:, None, None], N)
    logdet = (P.logs.sum() + P.logdet_w_val * (C // N)) * P.x_len
    h0 = (torch.einsum("hc,bct->bht", P.W_start, y[:, :half]) + P.b_start[None, :, None]) * m3
    val = {"y": y, "h0": h0, "logdet_prev": ld_prev, "logdet": logdet, "_z": z, "_a": a, "_el": el, "_l": l}
    if not want_scale:
        return val, None
    with torch.no_grad():
        s_z = torch.cat([P.y_prev[:, :half].abs(), (out[:, :half].abs() + el * P.y_prev[:, half:].abs() * (1 + l.abs())) * m3], 1)
        s_a = (P.bias.abs()[None, :, None] + e * s_z * (1 + P.logs.abs())[None, :, None]) * m3
        s_y = _ungrp(torch.einsum("ok,bkgt->bogt", P.W.abs(), _grp(s_a, N)) * P.mask[:, None, None], N)
        s_h0 = (torch.einsum("hc,bct->bht", P.W_start.abs(), y[:, :half].abs()) + P.b_start.abs()[None, :, None]) * m3
        scale = {"y": s_y, "h0": s_h0, "logdet_prev": P.ld0.abs() + (l.abs() * m3).sum((1, 2)),
                 "logdet": (P.logs.abs().sum() + P.logdet_w.abs() * (C // N)) * P.x_len}
    return val, scale


def _params(I, dt, W=None):
    P = types.SimpleNamespace(B=I.B, C=I.C, H=I.H, T=I.T, N=I.N)
    for k in ("skip", "y_prev", "dx_wn", "dy_next", "W_end", "W_end_bwd", "b_end", "W_start", "b_start", "logs", "bias", "w_inv",
              "logdet_w", "out_prev", "dlogdet", "ld0", "dlogs0", "dbias0", "dw0", "mask", "x_len"):
        setattr(P, k, getattr(I, k).to(dt).clone())
    P.W = (I.W if W is None else W).to(dt).clone()
    P.logdet_w_val = P.logdet_w[0]
    return P


@functools.lru_cache(maxsize=None)
def _fwd_ref(kind, row, sig, dt, w_form="w"):
    """{name: (value, scale)} of the forward's five outputs in dtype dt."""
    I = _inputs(kind, *row)
    P = _params(I, dt, W={"w": I.W, "wT": I.W.T.contiguous()}[w_form])
    out = torch.einsum("ch,bht->bct", P.W_end, P.skip) + P.b_end[None, :, None]
    s_out = torch.einsum("ch,bht->bct", P.W_end.abs(), P.skip.abs()) + P.b_end.abs()[None, :, None]
    val, scale = _flow(P, out, sig, want_scale=True)
    res = {"out": (out, s_out)}
    res.update({k: (val[k], scale[k]) for k in ("y", "h0", "logdet_prev", "logdet")})
    return res


@functools.lru_cache(maxsize=None)
def _bwd_ref(kind, row, sig, mask_dskip, with_dld, dt, w_form="w"):
    """{name: (value, scale)} of the backward's outputs in dtype dt: autograd over _flow with out_prev a leaf."""
    I = _inputs(kind, *row)
    P = _params(I, dt, W={"w": I.W, "wT": I.W.T.contiguous()}[w_form])
    N, C, half, m3 = P.N, P.C, P.C // 2, P.mask[:, None]
    leaves = [P.y_prev, P.out_prev, P.logs, P.bias, P.W]
    for t in leaves:
        t.requires_grad_(True)
    # log det W: the value is the ABI's argument, the derivative is that of the true log-determinant
    true_ld = torch.logdet(P.W)
    P.logdet_w_val = P.logdet_w[0] + (true_ld - true_ld.detach())
    val, _ = _flow(P, P.out_prev, sig)
    dld = P.dlogdet if with_dld else torch.zeros_like(P.dlogdet)
    l1 = (val["y"] * P.dy_next).sum() + (val["h0"] * P.dx_wn).sum() + (dld * val["logdet_prev"]).sum()
    l2 = (dld * val["logdet"]).sum()
    dy_prev, dout_prev, p_dlogs, p_dbias, p_dw = torch.autograd.grad(l1, leaves, retain_graph=True)
    f_dlogs, f_dw = torch.autograd.grad(l2, [P.logs, P.W]) if with_dld else (torch.zeros_like(p_dlogs), torch.zeros_like(p_dw))
    with torch.no_grad():
        dskip = torch.einsum("ch,bct->bht", P.W_end_bwd, dout_prev)
        s_dskip = torch.einsum("ch,bct->bht", P.W_end_bwd.abs(), dout_prev.abs())
        if mask_dskip:
            dskip, s_dskip = dskip * m3, s_dskip * m3
        # the same chain on absolute values
        z, a, el, l = val["_z"].detach(), val["_a"].detach(), val["_el"].detach(), val["_l"].detach()
        e = torch.exp(P.logs)[None, :, None] * (1 + P.logs.abs())[None, :, None]
        s_g = P.dy_next.abs().clone()
        s_g[:, :half] += torch.einsum("hc,bht->bct", P.W_start.abs(), (P.dx_wn * m3).abs())
        s_gz = _grp(s_g * m3, N)                                                       # (B, N, G, T)
        s_dym = _ungrp(torch.einsum("ok,bogt->bkgt", P.W.abs(), s_gz), N) * m3         # gradient of a
        s_dz = s_dym * e
        y1 = P.y_prev[:, half:].abs()
        lr = P.out_prev[:, half:]
        if sig:
            sg = torch.sigmoid(lr + 2.0)
            fac = sg * (1 - sg) / (1e-6 + sg) * (1 + lr.abs())
        else:
            fac = torch.ones_like(lr)
        s_dl = (s_dz[:, half:] * el * (1 + l.abs()) * y1 + dld.abs()[:, None, None]) * m3 * fac
        s_dy = torch.cat([s_dz[:, :half], s_dz[:, half:] * el * (1 + l.abs()) * m3], 1)
        s_dout = torch.cat([s_dz[:, half:] * m3, s_dl], 1)
        tt = (dld.abs() * P.x_len).sum()
        sp_dlogs, sp_dbias = (s_dz * z.abs()).sum((0, 2)), s_dym.sum((0, 2))
        sp_dw = torch.einsum("bogt,bkgt->ok", s_gz, _grp(a.abs(), N))
        res = {"dy_prev": (dy_prev, s_dy), "dout_prev": (dout_prev, s_dout), "dskip": (dskip, s_dskip),
               "part_dlogs": (p_dlogs, sp_dlogs), "part_dbias": (p_dbias, sp_dbias), "part_dw": (p_dw, sp_dw),
               "dlogs": (P.dlogs0 + p_dlogs + f_dlogs, P.dlogs0.abs() + sp_dlogs + tt),
               "dbias": (P.dbias0 + p_dbias, P.dbias0.abs() + sp_dbias),
               "dw": (P.dw0 + p_dw + f_dw, P.dw0.abs() + sp_dw + P.w_inv.T.abs() * (C // N) * tt)}
    return {k: (v.detach(), s.detach()) for k, (v, s) in res.items()}


# =============================================================================================== the launches
def _fwd_args(D, I, null=None):
    B, C, H, T = I.B, I.C, I.H, I.T
    t = {"skip": I.skip, "wp_end": pack_weight(I.W_end), "b_end": I.b_end, "y_prev": I.y_prev, "mask": I.mask, "logs": I.logs,
         "bias": I.bias, "w": I.W, "logdet_w": I.logdet_w, "x_len": I.x_len, "wp_start": pack_weight(I.W_start), "b_start": I.b_start}
    args = [None if k == null else D.inp(k, v) for k, v in t.items()]
    outs = [("out", (B, C, T), None), ("y", (B, C, T), None), ("h0", (B, H, T), None), ("logdet_prev", (B,), I.ld0), ("logdet", (B,), None)]
    return args + [None if k == null else D.out(k, s, init=i) for k, s, i in outs]


def _launch_fwd(G, I, sig):
    D = Dev()
    G.hip.call("glowtts_flow_boundary_fwd", *_fwd_args(D, I), I.B, I.C, I.H, I.T, I.N, sig)
    return D.finish()


def _n_partial(B, C, T, N):
    return B * ((T + 31) // 32) * (C // N) * (2 * N + N * N)


def _bwd_args(D, I, with_dld=True, null=None):
    B, C, H, T = I.B, I.C, I.H, I.T
    t = {"dx_wn": I.dx_wn, "wb_start": pack_weight(I.W_start.T.contiguous()), "dy_next": I.dy_next, "y_prev": I.y_prev,
         "out_prev": I.out_prev, "mask": I.mask, "logs": I.logs, "bias": I.bias, "w": I.W, "dlogdet": I.dlogdet if with_dld else None,
         "wb_end": pack_weight(I.W_end_bwd.T.contiguous())}
    args = [None if k == null else D.inp(k, v) for k, v in t.items()]
    outs = [("dy_prev", (B, C, T)), ("dout_prev", (B, C, T)), ("dskip", (B, H, T)), ("partial", (_n_partial(B, C, T, 4) * 2,))]
    return args + [None if k == null else D.out(k, s) for k, s in outs]


def _ungroup_vec(v, N):
    """[k][g] -> channel order."""
    return _ungrp(v[None, :, :, None], N)[0, :, 0]


def _launch_bwd(G, I, sig, mask_dskip, with_dld=True):
    """Both launches; the partial buffer of the first is handed to the second as it stands."""
    B, C, H, T, N = I.B, I.C, I.H, I.T, I.N
    D = Dev()
    G.hip.call("glowtts_flow_boundary_bwd", *_bwd_args(D, I, with_dld), B, C, H, T, N, sig, mask_dskip)
    got = D.finish()
    n, nv, g = _n_partial(B, C, T, N), 2 * N + N * N, C // N
    part = got.pop("partial")
    assert bool((part[n:] == GUARD[torch.float32]).all()), "written beyond the partials"
    assert not bool((part[:n] == GUARD[torch.float32]).any()), "a partial was left unwritten"
    psum = part[:n].double().reshape(-1, g, nv).sum(0)                                 # [g][v]
    got["part_dlogs"], got["part_dbias"] = _ungroup_vec(psum[:, :N].T, N), _ungroup_vec(psum[:, N:2 * N].T, N)
    got["part_dw"] = psum[:, 2 * N:].sum(0).reshape(N, N)
    R = Dev()
    G.hip.call("glowtts_flow_boundary_bwd_reduce", R.inp("partial", part[:n].contiguous()), R.inp("w_inv", I.w_inv) if with_dld else None,
               R.inp("dlogdet", I.dlogdet) if with_dld else None, R.inp("x_len", I.x_len), R.out("dlogs", (C,), init=I.dlogs0),
               R.out("dbias", (C,), init=I.dbias0), R.out("dw", (N, N), init=I.dw0), B, C, T, N)
    red = R.finish()
    got.update({k: red[k] for k in ("dlogs", "dbias", "dw")})
    return got


def _check(what, got, ref, names, exact=()):
    for name in names:
        want, scale = ref[name]
        assert bool(torch.isfinite(got[name]).all()), f"{what} {name}: non-finite output"
        key = name.replace("part_", "")
        fig = units(got[name], want, scale)
        print(f"{what} {name}: {fig:.2f} u (bound {BOUNDS[key]})")
        assert fig <= BOUNDS[key], f"{what} {name}: {fig:.2f} u > {BOUNDS[key]} u"
        if name in exact:
            assert torch.equal(got[name].double(), want), f"{what} {name}: differs from exact arithmetic"


# =============================================================================================== 1. forward
@gpu
@pytest.mark.parametrize("sig", [0, 1])
@pytest.mark.parametrize("row", ROW_PARAMS)
def test_boundary_fwd(G, row, sig):
    """out, y, h0, logdet_prev (accumulated onto a non-zero start) and logdet, each against fp64; y and h0 are exactly 0 beyond an
    utterance's end (their scale is 0 there), out is not masked.  Counting inputs: out, y, h0 EQUAL."""
    I = _inputs("random", *row)
    _check(f"fwd {row} sig={sig}", _launch_fwd(G, I, sig), _fwd_ref("random", row, sig, torch.float64), FWD_OUT)
    if sig == 0:
        I = _inputs("count", *row)
        _check(f"fwd {row} count", _launch_fwd(G, I, 0), _fwd_ref("count", row, 0, torch.float64), FWD_OUT, exact=EXACT)


# =============================================================================================== 2. backward
@gpu
@pytest.mark.parametrize("mask_dskip", [0, 1])
@pytest.mark.parametrize("sig", [0, 1])
@pytest.mark.parametrize("row", ROW_PARAMS)
def test_boundary_bwd(G, row, sig, mask_dskip):
    """dy_prev, dout_prev, dskip, the partials' sums and dlogs / dbias / dw (ADDED to non-zero starts), each against fp64 autograd;
    on two rows also with dlogdet NULL in both launches (the reduce then adds the partials' sums alone).  Counting inputs: dy_prev,
    dout_prev, dskip EQUAL."""
    I = _inputs("random", *row)
    for with_dld in (True, False) if row in NULL_DLOGDET_ROWS else (True,):
        what = f"bwd {row} sig={sig} mask_dskip={mask_dskip} dlogdet={int(with_dld)}"
        _check(what, _launch_bwd(G, I, sig, mask_dskip, with_dld), _bwd_ref("random", row, sig, mask_dskip, with_dld, torch.float64), BWD_OUT)
    if sig == 0:
        I = _inputs("count", *row)
        _check(f"bwd {row} count mask_dskip={mask_dskip}", _launch_bwd(G, I, 0, mask_dskip),
               _bwd_ref("count", row, 0, mask_dskip, True, torch.float64), BWD_OUT, exact=EXACT)


# =============================================================================================== 3. the ABI's rejections
def _sized(B, C, H, T):
    """Random buffers of the sizes of shape (B, C, H, T) (weights and partials at least as large as any n_split needs): should an
    entry point launch after all, nothing is read or written out of bounds."""
    gen = torch.Generator().manual_seed(B + C + H + T)
    rn = lambda *shape: torch.randn(shape, generator=gen)                                   # noqa: E731
    return types.SimpleNamespace(B=B, C=C, H=H, T=T, N=4, skip=rn(B, H, T), y_prev=rn(B, C, T), dx_wn=rn(B, H, T), dy_next=rn(B, C, T),
                                 out_prev=rn(B, C, T), W_end=rn(C, H), W_end_bwd=rn(C, H), b_end=rn(C), W_start=rn(H, C), b_start=rn(H),
                                 logs=rn(C), bias=rn(C), W=rn(4, 4), w_inv=rn(4, 4), logdet_w=rn(1), dlogdet=rn(B), ld0=rn(B),
                                 x_len=rn(B), mask=rn(B, T), dlogs0=rn(C), dbias0=rn(C), dw0=rn(4, 4))


def _untouched(D, inits):
    torch.cuda.synchronize()
    for name, _shape, buf, lo, numel in D.outs:
        b = buf.cpu()
        if name in inits:
            assert torch.equal(b[lo:lo + numel], inits[name].reshape(-1)), f"{name} touched"
            b[lo:lo + numel] = GUARD[torch.float32]
        assert bool((b == GUARD[torch.float32]).all()), f"{name} touched"
    D.finish()


@gpu
def test_abi_rejects_before_any_launch(G):
    """n_split 3, C = 194, H = 193, C / n_split = 65, T % 4 != 0, a tensor one float off 16 bytes, a NULL pointer, reduce with
    dlogdet but without w_inv: an error code with glowtts_last_error set and no output touched.  B = 0 or T = 0: a no-op."""
    lib = G.hip.load()
    cases = [((2, 12, 8, 8, 3), {}, "n_split=3"), ((1, 194, 8, 8, 2), {}, "shape"), ((1, 8, 193, 8, 2), {}, "shape"),
             ((1, 130, 8, 8, 2), {}, "shape"), ((1, 8, 8, 6, 2), {}, "shape"), ((1, 8, 8, 8, 2), {"mis": True}, "16-byte aligned"),
             ((1, 8, 8, 8, 2), {"null": True}, "null pointer"), ((0, 8, 8, 8, 2), {}, None), ((2, 8, 8, 0, 2), {}, None)]
    for (B, C, H, T, N), kw, match in cases:
        I = _sized(max(B, 1), C, H, max(T, 4))             # (B = 0 / T = 0 are handed over as integers only)
        for entry in ("fwd", "bwd", "reduce"):
            mis = {"fwd": "y_prev", "bwd": "dskip"}.get(entry) if kw.get("mis") else None
            null = {"fwd": "b_end", "bwd": "wb_end", "reduce": "dbias"}[entry] if kw.get("null") else None
            if entry == "reduce" and (kw.get("mis") or match == "shape"):
                continue                                 # (the reduce entry reads no 16-byte vectors and has no limits of its own)
            D = Dev(mis)
            if entry == "fwd":
                call = ("glowtts_flow_boundary_fwd", *_fwd_args(D, I, null=null), B, C, H, T, N, 0)
                inits = {"logdet_prev": I.ld0}
            elif entry == "bwd":
                call = ("glowtts_flow_boundary_bwd", *_bwd_args(D, I, null=null), B, C, H, T, N, 0, 1)
                inits = {}
            else:
                inits = {"dlogs": I.dlogs0, "dbias": I.dbias0, "dw": I.dw0}
                outs = [None if k == null else D.out(k, v.shape, init=v) for k, v in inits.items()]
                call = ("glowtts_flow_boundary_bwd_reduce", D.inp("partial", torch.randn(_n_partial(I.B, C, I.T, 4) * 2)),
                        D.inp("w_inv", I.w_inv), D.inp("dlogdet", I.dlogdet), D.inp("x_len", I.x_len), *outs, B, C, T, N)
            if match is None:
                G.hip.call(*call)
            else:
                with pytest.raises(RuntimeError, match=match):
                    G.hip.call(*call)
                assert re.search(match, lib.glowtts_last_error().decode())
            _untouched(D, inits)
            print(f"{entry} {(B, C, H, T, N)} {kw}: {'no-op' if match is None else 'rejected'}")
    I = _sized(1, 8, 8, 8)
    D = Dev()
    inits = {"dlogs": I.dlogs0, "dbias": I.dbias0, "dw": I.dw0}
    with pytest.raises(RuntimeError, match="dlogdet given without w_inv"):
        G.hip.call("glowtts_flow_boundary_bwd_reduce", D.inp("partial", torch.randn(_n_partial(1, 8, 8, 2))), None, D.inp("dlogdet", I.dlogdet),
                   D.inp("x_len", I.x_len), *[D.out(k, v.shape, init=v) for k, v in inits.items()], 1, 8, 8, 2)
    _untouched(D, inits)


# =============================================================================================== 4. on the CPU
def _variants(row):
    for sig in (0, 1):
        yield "fwd", (sig,)
        for mask_dskip in (0, 1):
            for with_dld in (True, False) if row in NULL_DLOGDET_ROWS else (True,):
                yield "bwd", (sig, mask_dskip, with_dld)


def test_bound_table_matches_fp32_cpu_evaluation():
    """Every bound is 4 x the figure of the same formulas in fp32 torch on the CPU against fp64 (worst over ROWS and variants),
    rounded up to a power of two: fig <= bound <= 16 fig."""
    figs = {}
    for row, _why in ROWS:
        for which, v in _variants(row):
            ref = (_fwd_ref if which == "fwd" else _bwd_ref)("random", row, *v, torch.float64)
            got = (_fwd_ref if which == "fwd" else _bwd_ref)("random", row, *v, torch.float32)
            for name, (want, scale) in ref.items():
                key = name.replace("part_", "")
                figs[key] = max(figs.get(key, 0.0), units(got[name][0], want, scale))
    for key in BOUNDS:
        print(f"fp32 CPU {key}: {figs[key]:.2f} u (bound {BOUNDS[key]})")
    assert set(figs) == set(BOUNDS)
    for key, fig in figs.items():
        bound = BOUNDS[key]
        assert bound == 2 ** round(math.log2(bound)), key
        assert fig <= bound <= 16 * fig, (key, fig, bound)


def test_counting_inputs_are_exact_in_fp32_on_the_cpu():
    """On the counting inputs fp32 and fp64 torch agree in every output, and every sum of |terms| is below 2**24: what the GPU
    tests assert EQUAL is exact in fp32, whatever the order of the sums."""
    for row, _why in ROWS:
        for which, v in (("fwd", (0,)), ("bwd", (0, 0, True)), ("bwd", (0, 1, True))):
            fn = _fwd_ref if which == "fwd" else _bwd_ref
            ref, got = fn("count", row, *v, torch.float64), fn("count", row, *v, torch.float32)
            for name, (want, scale) in ref.items():
                assert torch.equal(got[name][0].double(), want), (row, name)
                assert torch.equal(want, want.round()) and float(scale.max()) < 2 ** 24, (row, name, float(scale.max()))
                if name in EXACT:
                    assert float(want.abs().max()) > 0, (row, name)


def test_counting_matrices_tell_w_from_its_transpose():
    """The counting W has det +1, is not symmetric and not its own inverse; being a signed permutation its inverse is its transpose.
    Every output that reads W changes on the counting inputs when W^T (= W^-1) takes its place."""
    for n in (2, 4):
        w = _signed_perm(n).double()
        assert torch.equal(w @ w.T, torch.eye(n, dtype=torch.float64)) and abs(float(torch.det(w)) - 1.0) < 1e-12
        assert not torch.equal(w, w.T) and not torch.equal(w @ w, torch.eye(n, dtype=torch.float64))
    for row, _why in ROWS:
        a, b = _fwd_ref("count", row, 0, torch.float64), _fwd_ref("count", row, 0, torch.float64, "wT")
        for name in ("y", "h0"):
            assert not torch.equal(a[name][0], b[name][0]), (row, name)
        a, b = _bwd_ref("count", row, 0, 1, True, torch.float64), _bwd_ref("count", row, 0, 1, True, torch.float64, "wT")
        for name in ("dy_prev", "dout_prev", "dskip", "dw"):
            assert not torch.equal(a[name][0], b[name][0]), (row, name)
