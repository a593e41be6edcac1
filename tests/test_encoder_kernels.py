"""The channel LayerNorm of csrc/norm.hip and the phoneme embedding of csrc/train_ops.hip through the C ABI
(glow_tts_train._hip.call), against plain fp64 torch on the CPU written from the header's formulas; nothing of the package is used.
The GPU tests are marked `gpu`; the tests at the end of the module check the bound table and the spread of the variants on the CPU.

Every launch (tests/helpers.py: Dev): each input is a copy inside a guarded buffer and must be bit-identical afterwards; each
output lives between guard sentinels that must survive and is pre-filled with the sentinel; the accumulated outputs (dgamma, dbeta,
dweight) start from known non-zero values.  Lengths are ragged; from two utterances on, one has length 0; inputs beyond an
utterance's end hold random finite values and are NOT masked.

LayerNorm: glowtts_chan_layernorm_fwd_act / _bwd_act (the `_ex` and plain forms once each: the `_act` form with neutral flags, bit
for bit).    v = f(x) mask_x + res keep drop_scale, f = ReLU when relu_in ; mean, var over the channels ; rstd = (var + eps)^-1/2 ;
             y = okeep oscale relu_out(gamma (v - mean) rstd + beta) ; stats = (mean, rstd)
backward: fp64 autograd of <y, dy> for dx, dres, dgamma, dbeta (ADDED to non-zero starts); it is handed the fp64 stats and y rounded
to fp32.  Shapes (B, C, T): LN_SHAPES, the four instantiations (8, 24, 32 and 96 channels per thread) at both sides of each
dispatch edge.  Variants: LN_VARIANTS, spread over the shapes by LN_PLAN so that every instantiation sees every one.
gamma and beta are +-[0.5, 1.5], gamma with one exact zero; a tenth of x is exactly 0 (the relu_in gate must be closed there);
column (0, :, 1) holds equal small integers (x = 3, res = 2, kept); both dropout scales are 2.
Exact: y == post(beta) bit for bit (post = the output ReLU and dropout) where mask_x is 0 and there is no residual, in the column
of equal integers and in the channel whose gamma is 0; where a keep byte is 0 the output (y) or gradient (dres) is exactly 0; dx is
exactly 0 where mask_x is 0 and, under relu_in, where x <= 0.
Bounds in u = 2**-24 times a scale, 4 x the fp32 CPU figure rounded up to a power of two, as in tests/test_boundary_kernels.py:
    output    scale                                                                 fp32 CPU    bound    MI355X
    y         |gamma| |xhat| + |beta| (times oscale where kept)                     3.67 u      16 u     4.85 u
    mean      mean_c |v|                                                            2.44 u      16 u     2.60 u
    rstd      rstd                                                                  3.01 u      16 u     3.75 u
    dx, dres  rstd (|g| + mean_c |g| + |xhat| mean_c |g xhat|), g = dy' gamma       3.69 u      16 u     2.82 u
    dgamma    |start| + sum |dy' xhat|                                              3.94 u      16 u     2.74 u
    dbeta     |start| + sum |dy'|                                                   2.61 u      16 u     2.07 u

Embedding: glowtts_embed_fwd / _bwd.  Shapes (B, T, H, V): EMB_SHAPES.  Forward: one fp32 multiplication per element, asserted
EQUAL to fp32 torch; the columns of the ids -1 and V are all NaN and their neighbours untouched.  Backward: against an fp64 segment
sum in u times |start| + |scale| sum |dout| (fp32 CPU 2.16 u, bound 16 u, MI355X 2.16 u); dweight starts non-zero; the last vocabulary
row is named by no id and keeps its start bit for bit; the out-of-range ids contribute nothing.  Counting dout (small integers,
scale 2): EQUAL.
"""
import functools
import math
import re
import types

import pytest
import torch

from helpers import Dev, GUARD, bits_equal, units

gpu = pytest.mark.gpu

EPS = 1e-4
LN_SHAPES = [((2, 5, 33), 8, "C below one slice set; a second, one-frame tile"),
             ((2, 64, 32), 8, "CPT 8 / 24 edge"), ((2, 65, 7), 24, "CPT 8 / 24 edge"),
             ((1, 192, 33), 24, "CPT 24 / 32 edge"), ((2, 193, 4), 32, "CPT 24 / 32 edge"),
             ((1, 256, 33), 32, "CPT 32 / 96 edge"), ((1, 257, 5), 96, "CPT 32 / 96 edge"),
             ((1, 768, 33), 96, "the maximum"),
             ((3, 600, 9), 96, "the parameter kernel's second slab holds one utterance")]
LN_VARIANTS = {                                           # res, mask_x, drop (with dres), dres, relu_in, relu_out, odrop, stats
    "plain":      dict(res=0, mask=0, drop=0, dres=0, relu_in=0, relu_out=0, odrop=0, stats=0),   # dres NULL without drop; stats NULL
    "res_mask":   dict(res=1, mask=1, drop=0, dres=1, relu_in=0, relu_out=0, odrop=0, stats=1),
    "drop":       dict(res=1, mask=1, drop=1, dres=1, relu_in=0, relu_out=0, odrop=0, stats=1),
    "relu_in":    dict(res=0, mask=1, drop=0, dres=0, relu_in=1, relu_out=0, odrop=0, stats=1),
    "relu_out":   dict(res=1, mask=0, drop=0, dres=0, relu_in=0, relu_out=1, odrop=0, stats=1),
    "relu_odrop": dict(res=0, mask=1, drop=0, dres=0, relu_in=0, relu_out=1, odrop=1, stats=0)}
ALL = tuple(LN_VARIANTS)
LN_PLAN = {(2, 5, 33): ("plain", "res_mask", "drop"), (2, 64, 32): ("relu_in", "relu_out", "relu_odrop"),
           (2, 65, 7): ALL, (1, 192, 33): ("res_mask", "relu_out"),
           (2, 193, 4): ALL, (1, 256, 33): ("drop", "relu_odrop"),
           (1, 257, 5): ("plain", "relu_in"), (1, 768, 33): ("res_mask", "relu_odrop"), (3, 600, 9): ALL}
LN_PARAMS = [pytest.param(s, id="x".join(map(str, s))) for s, _cpt, _why in LN_SHAPES]
LN_BOUNDS = {"y": 16, "mean": 16, "rstd": 16, "dx": 16, "dgamma": 16, "dbeta": 16}      # in u: the table of the module docstring

EMB_SHAPES = [((1, 1, 1, 1), "the smallest"), ((2, 67, 5, 7), "a second forward tile of three frames"),
              ((1, 40, 256, 3), "the backward's lane-loop edge"), ((1, 40, 257, 3), "the backward's lane-loop edge"),
              ((1, 8, 1024, 2), "the maximum H"),
              ((3, 700, 8, 3), "2100 positions, so a second, 52-position chunk; one token holds more than 256 positions of one chunk, "
                               "whole compaction rounds among them")]
EMB_PARAMS = [pytest.param(s, id="x".join(map(str, s))) for s, _why in EMB_SHAPES]
EMB_BOUND = 16                                            # in u


@pytest.fixture(scope="module")
def G():
    from glow_tts_train import _hip

    _hip.load()
    return types.SimpleNamespace(hip=_hip)


# =============================================================================================== LayerNorm: inputs, reference
@functools.lru_cache(maxsize=None)
def _ln_inputs(B, C, T):
    gen = torch.Generator().manual_seed(7919 * B + 104729 * C + T)
    I = types.SimpleNamespace(B=B, C=C, T=T)
    lengths = torch.tensor([T, 0, max(1, T - 3)][:B]) if B >= 2 else torch.tensor([T - 2])
    I.lengths = lengths
    I.mask = (torch.arange(T)[None] < lengths[:, None]).float()
    rn = lambda *shape: torch.randn(shape, generator=gen)                                   # noqa: E731
    pm = lambda n: (torch.rand(n, generator=gen) + 0.5) * (torch.randint(0, 2, (n,), generator=gen) * 2 - 1).float()   # noqa: E731
    I.x, I.res, I.dy = rn(B, C, T), rn(B, C, T), rn(B, C, T)
    I.x[torch.rand(B, C, T, generator=gen) < 0.1] = 0.0
    I.drop = (torch.rand(B, C, T, generator=gen) < 0.5).to(torch.uint8)
    I.odrop = (torch.rand(B, C, T, generator=gen) < 0.5).to(torch.uint8)
    I.x[0, :, 1], I.res[0, :, 1], I.drop[0, :, 1] = 3.0, 2.0, 1                  # a column of equal small integers
    I.gamma, I.beta = pm(C), pm(C)
    I.zero_c = C // 2
    I.gamma[0], I.gamma[C - 1] = I.gamma[0].abs(), -I.gamma[C - 1].abs()      # both signs, whatever the draw
    I.gamma[I.zero_c] = 0.0
    assert bool((I.gamma > 0).any()) and bool((I.gamma < 0).any())
    I.dgamma0, I.dbeta0 = rn(C), rn(C)
    I.drop_scale = I.oscale = 2.0
    return I


@functools.lru_cache(maxsize=None)
def _ln_ref(shape, vname, dt):
    """{name: (value, scale)} of y, mean, rstd, dx, dres, dgamma, dbeta in dtype dt: the header's formulas and their autograd."""
    I, V = _ln_inputs(*shape), LN_VARIANTS[vname]
    c = lambda t: t.to(dt).clone()                                                          # noqa: E731
    x, res, gamma, beta, dy = c(I.x), c(I.res), c(I.gamma), c(I.beta), c(I.dy)
    leaves = [x, res, gamma, beta]
    for t in leaves:
        t.requires_grad_(True)
    m = c(I.mask)[:, None] if V["mask"] else torch.ones(I.B, 1, I.T, dtype=dt)
    keep = c(I.drop) * I.drop_scale if V["drop"] else torch.ones(shape, dtype=dt)
    okeep = c(I.odrop) * I.oscale if V["odrop"] else torch.ones(shape, dtype=dt)
    v = (torch.relu(x) if V["relu_in"] else x) * m
    if V["res"]:
        v = v + res * keep
    mean = v.mean(1, keepdim=True)
    var = ((v - mean) ** 2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + EPS)
    xhat = (v - mean) * rstd
    y0 = gamma[None, :, None] * xhat + beta[None, :, None]
    y = (torch.relu(y0) if V["relu_out"] else y0) * okeep
    dx, dres, dgamma, dbeta = torch.autograd.grad((y * dy).sum(), leaves, allow_unused=True)
    with torch.no_grad():
        dyp = dy * okeep * ((y0 > 0).to(dt) if V["relu_out"] else 1.0)
        g = (dyp * gamma[None, :, None]).abs()
        s_dv = rstd * (g + g.mean(1, keepdim=True) + xhat.abs() * (g * xhat.abs()).mean(1, keepdim=True))
        gate = m * ((x > 0).to(dt) if V["relu_in"] else 1.0)
        res_ = {"y": (y, (gamma.abs()[None, :, None] * xhat.abs() + beta.abs()[None, :, None]) * okeep),
                "mean": (mean[:, 0], v.abs().mean(1)), "rstd": (rstd[:, 0], rstd[:, 0]),
                "dx": (dx, s_dv * gate),
                "dgamma": (c(I.dgamma0) + dgamma, c(I.dgamma0).abs() + (dyp * xhat).abs().sum((0, 2))),
                "dbeta": (c(I.dbeta0) + dbeta, c(I.dbeta0).abs() + dyp.abs().sum((0, 2)))}
        if V["res"]:
            res_["dres"] = (dres, s_dv * keep)
    return {k: (a.detach(), s.detach()) for k, (a, s) in res_.items()}


def _post_beta(I, V):
    """fp32: what y is, exactly, wherever the normalised value is exactly 0 or gamma is 0."""
    pb = I.beta[None, :, None].expand(I.B, I.C, I.T)
    if V["relu_out"]:
        pb = torch.relu(pb)
    if V["odrop"]:
        pb = torch.where(I.odrop.bool(), pb * I.oscale, torch.zeros(()))
    return pb.contiguous()


# =============================================================================================== LayerNorm: the launches
def _ln_fwd(G, I, V, form="act", stats=None):
    B, C, T = I.B, I.C, I.T
    D = Dev()
    head = [D.inp("x", I.x), D.inp("res", I.res) if V["res"] else None]
    ex = [D.inp("mask_x", I.mask) if V["mask"] else None, D.inp("drop", I.drop) if V["drop"] else None, I.drop_scale if V["drop"] else 1.0]
    tail = [D.inp("gamma", I.gamma), D.inp("beta", I.beta), D.out("y", (B, C, T)),
            D.out("stats", (B, 2, T)) if (V["stats"] if stats is None else stats) else None]
    if form == "act":
        G.hip.call("glowtts_chan_layernorm_fwd_act", *head, *ex, *tail, V["relu_in"], V["relu_out"],
                   D.inp("odrop", I.odrop) if V["odrop"] else None, I.oscale if V["odrop"] else 1.0, B, C, T, EPS)
    elif form == "ex":
        G.hip.call("glowtts_chan_layernorm_fwd_ex", *head, *ex, *tail, B, C, T, EPS)
    else:
        G.hip.call("glowtts_chan_layernorm_fwd", *head, *tail, B, C, T, EPS)
    return D.finish()


def _ln_bwd(G, I, V, ref, form="act"):
    """The backward is handed the reference's stats and y, rounded to fp32."""
    B, C, T = I.B, I.C, I.T
    D = Dev()
    stats = torch.stack([ref["mean"][0], ref["rstd"][0]], 1).float().contiguous()
    head = [D.inp("x", I.x), D.inp("res", I.res) if V["res"] else None]
    ex = [D.inp("mask_x", I.mask) if V["mask"] else None, D.inp("drop", I.drop) if V["drop"] else None, I.drop_scale if V["drop"] else 1.0]
    mid = [D.inp("gamma", I.gamma), D.inp("stats", stats)]
    dy = D.inp("dy", I.dy)
    outs = lambda with_dres: [D.out("dx", (B, C, T)), D.out("dres", (B, C, T)) if with_dres else None,   # noqa: E731
                              D.out("dgamma", (C,), init=I.dgamma0), D.out("dbeta", (C,), init=I.dbeta0)]
    if form == "act":
        G.hip.call("glowtts_chan_layernorm_bwd_act", *head, *ex, *mid, D.inp("y", ref["y"][0].float()) if V["relu_out"] else None, dy,
                   V["relu_in"], V["relu_out"], D.inp("odrop", I.odrop) if V["odrop"] else None, I.oscale if V["odrop"] else 1.0,
                   *outs(V["dres"]), B, C, T)
    elif form == "ex":
        G.hip.call("glowtts_chan_layernorm_bwd_ex", *head, *ex, *mid, dy, *outs(V["dres"]), B, C, T)
    else:
        o = outs(False)
        G.hip.call("glowtts_chan_layernorm_bwd", *head, *mid, dy, o[0], o[2], o[3], B, C, T)
    return D.finish()


def _ln_check(what, got, ref, names):
    for name in names:
        want, scale = ref[name]
        assert bool(torch.isfinite(got[name]).all()), f"{what} {name}: non-finite output"
        key = "dx" if name == "dres" else name
        fig = units(got[name], want, scale)
        print(f"{what} {name}: {fig:.2f} u (bound {LN_BOUNDS[key]})")
        assert fig <= LN_BOUNDS[key], f"{what} {name}: {fig:.2f} u > {LN_BOUNDS[key]} u"


# =============================================================================================== 1. LayerNorm
@gpu
@pytest.mark.parametrize("shape", LN_PARAMS)
def test_layernorm_fwd(G, shape):
    """y and stats (mean, rstd) against fp64, with and without stats; y == post(beta) bit for bit where the normalised column is
    constant (mask_x 0 without residual, the column of equal integers) and in the channel whose gamma is 0; y == 0 where the
    output's keep byte is 0."""
    I = _ln_inputs(*shape)
    for vname in LN_PLAN[shape]:
        V, ref = LN_VARIANTS[vname], _ln_ref(shape, vname, torch.float64)
        got = _ln_fwd(G, I, V)
        what = f"layernorm_fwd {shape} {vname}"
        if V["stats"]:
            got["mean"], got["rstd"] = got["stats"][:, 0], got["stats"][:, 1]
        _ln_check(what, got, ref, ("y", "mean", "rstd") if V["stats"] else ("y",))
        pb, y = _post_beta(I, V), got["y"]
        const = torch.zeros(I.B, I.T, dtype=torch.bool)
        const[0, 1] = True
        if V["mask"] and not V["res"]:
            const |= I.mask == 0
        assert bits_equal(y.transpose(1, 2)[const], pb.transpose(1, 2)[const]), what + ": y != beta in a constant column"
        assert bits_equal(y[:, I.zero_c], pb[:, I.zero_c]), what + ": y != beta where gamma is 0"
        if V["odrop"]:
            assert bool((y[I.odrop == 0] == 0).all()), what + ": a dropped element is not 0"


@gpu
@pytest.mark.parametrize("shape", LN_PARAMS)
def test_layernorm_bwd(G, shape):
    """dx, dres, dgamma, dbeta (the last two ADDED to non-zero starts) against fp64 autograd; dres == 0 where the residual's keep byte
    is 0; dx == 0 where mask_x is 0 and, under relu_in, where x <= 0 (x == 0 included)."""
    I = _ln_inputs(*shape)
    for vname in LN_PLAN[shape]:
        V, ref = LN_VARIANTS[vname], _ln_ref(shape, vname, torch.float64)
        got = _ln_bwd(G, I, V, ref)
        what = f"layernorm_bwd {shape} {vname}"
        _ln_check(what, got, ref, ("dx", "dgamma", "dbeta") + (("dres",) if V["dres"] else ()))
        if V["drop"]:
            assert bool((got["dres"][I.drop == 0] == 0).all()), what + ": dres != 0 at a dropped element"
        if V["mask"]:
            assert bool((got["dx"].transpose(1, 2)[I.mask == 0] == 0).all()), what + ": dx != 0 where mask_x is 0"
        if V["relu_in"]:
            assert int((I.x == 0).sum()) > 0 and bool((got["dx"][I.x <= 0] == 0).all()), what + ": the gate is open at x <= 0"


@gpu
def test_layernorm_ex_and_plain_forms_are_the_act_form(G):
    """glowtts_chan_layernorm_{fwd,bwd}_ex and the plain forms give, bit for bit, what the `_act` form gives with neutral flags
    (one utterance: one parameter slab, so the accumulation order is fixed)."""
    shape = (1, 192, 33)
    I = _ln_inputs(*shape)
    for vname, form in (("drop", "ex"), ("relu_out", "plain")):
        V = dict(LN_VARIANTS[vname], relu_out=0, dres=LN_VARIANTS[vname]["drop"])
        ref = _ln_ref(shape, vname, torch.float64)                                       # (only its stats are used)
        a, b = _ln_fwd(G, I, V, "act"), _ln_fwd(G, I, V, form)
        assert bits_equal(a["y"], b["y"]) and bits_equal(a["stats"], b["stats"]), form
        a, b = _ln_bwd(G, I, V, ref, "act"), _ln_bwd(G, I, V, ref, form)
        assert set(a) == set(b) and all(bits_equal(a[k], b[k]) for k in a), form
        print(f"layernorm {form} == act: {sorted(a)}")


@gpu
def test_layernorm_rejects_before_any_launch(G):
    """C = 769, drop without res (forward and backward), relu_out without y: an error code, nothing written."""
    lib = G.hip.load()
    for C, kw, match in ((769, {}, "C <= 768"), (8, {"drop_no_res": 1}, "bad shape"), (8, {"relu_no_y": 1}, "relu_out needs y")):
        B, T = 1, 8
        t = lambda *s: torch.randn(*s)                                                      # noqa: E731
        for which in ("fwd", "bwd"):
            if which == "fwd" and kw.get("relu_no_y"):
                continue
            D = Dev()
            res = None if kw.get("drop_no_res") else D.inp("res", t(B, C, T))
            drop = D.inp("drop", torch.ones(B, C, T, dtype=torch.uint8)) if kw.get("drop_no_res") else None
            inits = {"dgamma": t(C), "dbeta": t(C)}
            if which == "fwd":
                call = ("glowtts_chan_layernorm_fwd_act", D.inp("x", t(B, C, T)), res, None, drop, 2.0, D.inp("gamma", t(C)), D.inp("beta", t(C)),
                        D.out("y", (B, C, T)), D.out("stats", (B, 2, T)), 0, 0, None, 1.0, B, C, T, EPS)
            else:
                call = ("glowtts_chan_layernorm_bwd_act", D.inp("x", t(B, C, T)), res, None, drop, 2.0, D.inp("gamma", t(C)),
                        D.inp("stats", t(B, 2, T)), None, D.inp("dy", t(B, C, T)), 0, int(bool(kw.get("relu_no_y"))), None, 1.0,
                        D.out("dx", (B, C, T)), D.out("dres", (B, C, T)), D.out("dgamma", (C,), init=inits["dgamma"]),
                        D.out("dbeta", (C,), init=inits["dbeta"]), B, C, T)
            with pytest.raises(RuntimeError, match=match):
                G.hip.call(*call)
            assert re.search(match, lib.glowtts_last_error().decode())
            for name, value in D.finish().items():
                assert torch.equal(value.reshape(-1), inits[name]) if name in inits else bool((value == GUARD[torch.float32]).all()), name


# =============================================================================================== embedding
@functools.lru_cache(maxsize=None)
def _emb_inputs(kind, B, T, H, V):
    gen = torch.Generator().manual_seed(7919 * B + 104729 * T + 31 * H + V + len(kind))
    I = types.SimpleNamespace(B=B, T=T, H=H, V=V)
    I.ids = torch.randint(0, max(1, V - 1), (B, T), generator=gen)              # the last vocabulary row is named by no id (V >= 2)
    if T >= 600:
        I.ids[0, :600] = 0                                                      # whole compaction rounds of one token
    I.bad = []
    if T >= 8:
        I.ids[0, 1], I.ids[B - 1, T - 2] = -1, V                                # outside the vocabulary
        I.bad = [(0, 1), (B - 1, T - 2)]
    I.weight, I.dw0 = torch.randn(V, H, generator=gen), torch.randn(V, H, generator=gen)
    if kind == "count":
        I.dout, I.scale = torch.randint(-3, 4, (B, H, T), generator=gen).float(), 2.0
        I.dw0 = I.dw0.round()
    else:
        I.dout, I.scale = torch.randn(B, H, T, generator=gen), float(torch.tensor(math.sqrt(H), dtype=torch.float32))
    return I


def _emb_bwd_ref(I, dt):
    """(dweight, scale): dweight[v][h] = start + scale * sum over the positions holding id v of dout[b][h][t]."""
    ids = I.ids.reshape(-1)
    ok = (ids >= 0) & (ids < I.V)
    rows = I.dout.to(dt).permute(0, 2, 1).reshape(-1, I.H)[ok]
    s = torch.zeros(I.V, I.H, dtype=dt).index_add_(0, ids[ok], rows)
    sa = torch.zeros(I.V, I.H, dtype=dt).index_add_(0, ids[ok], rows.abs())
    return I.dw0.to(dt) + s * I.scale, I.dw0.to(dt).abs() + sa * abs(I.scale)


@gpu
@pytest.mark.parametrize("shape", EMB_PARAMS)
def test_embed_fwd(G, shape):
    """out[b][h][t] = weight[ids[b][t]][h] * scale: EQUAL to fp32 torch; the columns of the ids -1 and V are NaN, all else untouched."""
    I = _emb_inputs("random", *shape)
    B, T, H, V = shape
    D = Dev()
    G.hip.call("glowtts_embed_fwd", D.inp("ids", I.ids), D.inp("weight", I.weight), I.scale, D.out("out", (B, H, T)), B, T, H, V)
    got = D.finish()["out"]
    want = (I.weight[I.ids.clamp(0, V - 1)] * torch.tensor(I.scale, dtype=torch.float32)).permute(0, 2, 1).contiguous()
    for b, t in I.bad:
        assert bool(torch.isnan(got[b, :, t]).all()), f"embed_fwd {shape}: id {int(I.ids[b, t])} gives no NaN column"
        got[b, :, t] = want[b, :, t]
    assert len(I.bad) == 2 or T < 8
    assert torch.equal(got, want), f"embed_fwd {shape}"
    print(f"embed_fwd {shape}: ==")


@gpu
@pytest.mark.parametrize("shape", EMB_PARAMS)
def test_embed_bwd(G, shape):
    """dweight against an fp64 segment sum, ADDED to a non-zero start; a row no id names keeps its start bit for bit; ids outside
    the vocabulary contribute nothing.  Counting dout: EQUAL."""
    B, T, H, V = shape
    for kind in ("random", "count"):
        I = _emb_inputs(kind, *shape)
        D = Dev()
        G.hip.call("glowtts_embed_bwd", D.inp("ids", I.ids), D.inp("dout", I.dout), I.scale, D.out("dweight", (V, H), init=I.dw0), B, T, H, V)
        got = D.finish()["dweight"]
        want, scale = _emb_bwd_ref(I, torch.float64)
        fig = units(got, want, scale)
        print(f"embed_bwd {shape} {kind}: {fig:.2f} u (bound {EMB_BOUND})")
        assert fig <= EMB_BOUND
        if V >= 2:
            assert not bool((I.ids == V - 1).any()) and bits_equal(got[V - 1], I.dw0[V - 1]), "an untouched vocabulary row changed"
        if kind == "count":
            assert float(scale.max()) < 2 ** 24 and torch.equal(got.double(), want), f"embed_bwd {shape}: differs from exact arithmetic"
    if T >= 600:
        hits = (_emb_inputs("random", *shape).ids.reshape(-1)[:2048] == 0)
        assert int(hits.sum()) > 256 and bool(hits[256:512].all()) and 2048 < B * T < 2048 + 256


@gpu
def test_embed_bwd_rejects_h_above_1024(G):
    lib = G.hip.load()
    B, T, H, V = 1, 4, 1025, 2
    D = Dev()
    dw0 = torch.randn(V, H)
    with pytest.raises(RuntimeError, match="H <= 1024"):
        G.hip.call("glowtts_embed_bwd", D.inp("ids", torch.zeros(B, T, dtype=torch.int64)), D.inp("dout", torch.randn(B, H, T)), 1.0,
                   D.out("dweight", (V, H), init=dw0), B, T, H, V)
    assert re.search("H <= 1024", lib.glowtts_last_error().decode())
    assert torch.equal(D.finish()["dweight"], dw0)


# =============================================================================================== on the CPU
def test_every_instantiation_sees_every_variant():
    """LN_PLAN spreads the variants so that each option appears at one shape of each instantiation at least; mask_x with an empty
    utterance in each."""
    assert set(LN_PLAN) == {s for s, _c, _w in LN_SHAPES}
    for cpt in (8, 24, 32, 96):
        shapes = [s for s, c, _w in LN_SHAPES if c == cpt]
        assert all((8 if s[1] <= 64 else 24 if s[1] <= 192 else 32 if s[1] <= 256 else 96) == cpt for s in shapes)
        seen = {v for s in shapes for v in LN_PLAN[s]}
        assert seen == set(LN_VARIANTS), (cpt, seen)
        assert any(LN_VARIANTS[v]["mask"] and int(_ln_inputs(*s).lengths.min()) == 0 for s in shapes for v in LN_PLAN[s]), cpt
    opt = lambda **kw: any(all(V[k] == x for k, x in kw.items()) for V in LN_VARIANTS.values())   # noqa: E731
    assert opt(res=0) and opt(res=1) and opt(mask=0) and opt(mask=1) and opt(drop=1, dres=1) and opt(drop=0, dres=0, res=1)
    assert opt(relu_in=1) and opt(relu_out=1, odrop=0) and opt(relu_out=1, odrop=1) and opt(stats=0)


def test_bound_table_matches_fp32_cpu_evaluation():
    """Every bound is 4 x the figure of the same formulas in fp32 torch on the CPU against fp64 (worst over the shapes and their
    variants), rounded up to a power of two: fig <= bound <= 16 fig."""
    figs = {}
    for shape, _cpt, _why in LN_SHAPES:
        for vname in LN_PLAN[shape]:
            ref, got = _ln_ref(shape, vname, torch.float64), _ln_ref(shape, vname, torch.float32)
            for name, (want, scale) in ref.items():
                key = "dx" if name == "dres" else name
                figs[key] = max(figs.get(key, 0.0), units(got[name][0], want, scale))
    bounds = dict(LN_BOUNDS)
    for shape, _why in EMB_SHAPES:
        I = _emb_inputs("random", *shape)
        want, scale = _emb_bwd_ref(I, torch.float64)
        figs["dweight"] = max(figs.get("dweight", 0.0), units(_emb_bwd_ref(I, torch.float32)[0], want, scale))
        J = _emb_inputs("count", *shape)
        assert torch.equal(_emb_bwd_ref(J, torch.float32)[0].double(), _emb_bwd_ref(J, torch.float64)[0])
    bounds["dweight"] = EMB_BOUND
    for key in bounds:
        print(f"fp32 CPU {key}: {figs[key]:.2f} u (bound {bounds[key]})")
    assert set(figs) == set(bounds)
    for key, fig in figs.items():
        bound = bounds[key]
        assert bound == 2 ** round(math.log2(bound)), key
        assert fig <= bound <= 16 * fig, (key, fig, bound)
