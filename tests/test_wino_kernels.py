"""The three kernels of csrc/convwino.hip one by one, through the C ABI (glow_tts_train._hip.call), against plain fp64 torch on the
CPU: wino_weights_kernel (glowtts_wino_weights), wino_gate_fwd_kernel (glowtts_conv_gate_fwd in "bf16x6+wrw" with U planes bound and
GLOWTTS_WINO = 1) and wino_bwd_kernel (glowtts_conv_fwd with the in-conv's backward pack, M = 192 rows from Cin = 384 channels, and
GLOWTTS_WINO_BWD = 1): the WN stack's gated 5-tap in-conv and its backward-data in Winograd F(4, 5) form.  tests/test_conv_math.py
and tests/test_wino_bwd_data.py compare max|err| / max|ref| over whole tensors of random data with ONE convolution at offset 0 of
the bound buffer: a wrong halo frame at one tile edge of one short utterance in a low-scale channel stays below that.  The GPU tests
are marked `gpu`; the others check the transforms, the bound table, the plans and the plane sizes on the CPU.

The form (csrc/convwino.hip):  out[m][4j + i] = sum_p AT[i][p] sum_c U[m][c][p] V[c][p][j],  U = G w (8 points from 5 taps),
V = BT d (8 points from the frames 4j - 2 .. 4j + 5, zero outside the utterance).  (AT, G, BT) are built here with `fractions` for the
points {0, 1, -1, 2, -2, 1/2, -1/2, inf} as tools/winograd_study.py does; test_transforms_are_the_5_tap_correlation asserts exactly
(in rationals, and in fp64) that AT ((G w) * (BT d)) is the correlation, so a wrong restatement cannot pass, and
test_g_rows_are_the_kernels pins the G rows that wino_weights_kernel spells out.  The fp64 REFERENCE of every output is the direct
convolution (F.conv1d on a zero-padded input), not the form.

Per-element scale: S[m][4j + i] = sum_p |AT[i][p]| sum_c |U[m][c][p]| |V[c][p][j]| in fp64 — the operand magnitude of the form; the
transforms amplify: on the rows' random inputs S is 4.0 to 4.8 x (median of a row) and at most 14.8 x the direct sum |w||x|.  Plain outputs (the backward) are measured in
u (S + |addend|), the gate outputs with the acts / tanh / sigmoid rows of the table of tests/test_conv_kernels.py with
S_pre = (S + |bias|) [drop_scale] + |cond|; U itself in u sum_k |G[p][k]| |w[k]|.  u = 2**-24.

Bounds: 4 x what the SAME form evaluated in fp32 torch on the CPU (transforms in fp32, the channel sum sequential in fp32, AT in
fp32, the gate with torch.tanh / torch.sigmoid) shows against fp64 on the tests' own random inputs, worst over the shape tables,
rounded up to a power of two (the margin 4: the project's for "sums in another order"), + SPLIT_EXTRA = 2 u for the plane split of
the products (tests/test_conv_kernels.py; U is stored as three planes that sum exactly: no extra).
test_bound_table_matches_fp32_cpu_evaluation recomputes the column and asserts fig <= bound <= 16 fig.
    output          fp32 CPU    bound     on the GPU    MI355X
    U                3.42 u     16 u        16 u       3.05 u
    y (backward)     1.73 u      8 u        10 u       0.88 u
    acts             1.86 u      8 u        10 u       1.27 u
    tanh             1.91 u      8 u        10 u       1.63 u
    sigmoid          2.10 u     16 u        18 u       1.65 u
(MI355X: the worst figure over the rows, profiles/r17_wino_wrw1_kernels.txt.)

Two kinds of input.
  1. Selection: one non-zero weight (1) per output row at a random (channel, tap), x integers in [-8, 8], bias 0, conditioning
     integers in [-2, 2], keep bytes 0 / 1 with drop_scale 2, integer addends: every pre-activation / output is ONE input value
     (times 2, plus an integer) or 0, taken by indexing.  The outputs are compared with the expected value (the forward: tanh and
     sigmoid of it) at SEL_TOL = 2**-10; the tests assert that SEL_TOL is at least the random bound on these inputs and below a
     quarter of the smallest gap between two distinct expected values (1): a frame of the neighbouring tile, utterance or channel is
     off by whole numbers.  (The fp32 form on the CPU deviates by at most 2.3e-5 on these inputs, the MI355X by 3.1e-5:
     test_selection_inputs_on_the_cpu.)
  2. Random: x ~ N(0, 1) times a channel scale exp(0.5 N), v ~ N (5 Cin)^-1/2, bias ~ 0.1 N, cond ~ 0.5 N, keep probability 0.7.

Every launch (tests/helpers.py: Dev): inputs are copies inside guarded buffers and must be bit-identical afterwards; outputs live
between guard sentinels; a strided y (the upper channel half of a (B, 2 M, T) tensor), a strided addend and a strided x are embedded
in buffers of sentinels / random values that must not change.  The packed weights lie at a NON-ZERO offset of the bound buffer
(behind a filler of 16 k floats; offsets that are no multiples of 80), the launch counters must advance by exactly 1 and a second
launch must give the same bits.  Frames beyond an utterance's length hold random finite values (the kernels have no mask_in);
masked outputs must be exactly 0.

Rows: FWD (B, H, T) and BWD (B, T) below, each with what it reaches: T / 4 < 16 (tiles of different utterances in neighbouring lanes of
a 16-lane DPP row: the halo must be zero, down to T = 4 where every tile is its own utterance), the halo loads of lanes 0 and 15, last
column groups of fewer than 48 / 32 tiles, one and two row groups, an empty utterance under mask_out.
"""
import ctypes
import functools
import math
import types
from fractions import Fraction as Fr

import pytest
import torch
import torch.nn.functional as F

from helpers import Dev, GUARD, U as EPS, bits_equal, units

gpu = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
BOUNDS = {"U": 16, "y": 8, "acts": 8, "th": 8, "sg": 16}      # in u: the table of the module docstring
SPLIT_EXTRA = 2          # u: the dropped cross products of the six-product form (tests/test_conv_kernels.py)
SEL_TOL = 2.0 ** -10
LDS_GATE, LDS_BWD = 147456, 98304
COLS_GATE, COLS_BWD = 48, 32
M_BWD, C_BWD = 192, 384


# =============================================================================================== the transforms
def _cook_toom():
    """(AT 4 x 8, G 8 x 5, BT 8 x 8) of F(4, 5) for the points 0, 1, -1, 2, -2, 1/2, -1/2 and infinity, as rationals."""
    pts = [Fr(0), Fr(1), Fr(-1), Fr(2), Fr(-2), Fr(1, 2), Fr(-1, 2)]
    m, r, n = 4, 5, 8

    def polymul(a, b):
        out = [Fr(0)] * (len(a) + len(b) - 1)
        for i, x in enumerate(a):
            for j, y in enumerate(b):
                out[i + j] += x * y
        return out

    def others(j):
        poly, norm = [Fr(1)], Fr(1)
        for k in range(n - 1):
            if k != j:
                poly, norm = polymul(poly, [-pts[k], Fr(1)]), norm * (pts[j] - pts[k] if j is not None else 1)
        return poly, norm

    AT = [[pts[j] ** i for j in range(n - 1)] + [Fr(int(i == m - 1))] for i in range(m)]
    G = [[pts[j] ** k / others(j)[1] for k in range(r)] for j in range(n - 1)] + [[Fr(0)] * (r - 1) + [Fr(1)]]
    BT = [others(j)[0] + [Fr(0)] for j in range(n - 1)] + [others(None)[0]]
    return AT, G, BT


AT_Q, G_Q, BT_Q = _cook_toom()
AT, GM, BT = (torch.tensor([[float(v) for v in row] for row in mat], dtype=F64) for mat in (AT_Q, G_Q, BT_Q))


def test_transforms_are_the_5_tap_correlation():
    """AT ((G w) * (BT d)) == sum_k w[k] d[i + k]: exactly, coefficient by coefficient, in rationals; and in fp64 on random data."""
    for k in range(5):
        for j in range(8):
            for i in range(4):
                got = sum(AT_Q[i][p] * G_Q[p][k] * BT_Q[p][j] for p in range(8))
                assert got == (1 if j == i + k else 0), (i, k, j, got)
    gen = torch.Generator().manual_seed(1)
    w, d = torch.randn(5, generator=gen, dtype=F64), torch.randn(8, generator=gen, dtype=F64)
    want = torch.stack([(w * d[i: i + 5]).sum() for i in range(4)])
    assert float((AT @ ((GM @ w) * (BT @ d)) - want).abs().max()) < 1e-12


def test_g_rows_are_the_kernels():
    """The rows wino_weights_kernel writes out: -w0 and w4 at the points 0 and infinity, -2/9 at +-1, 1/90, 2/45, .. at +-2 and
    32/45, .. at +-1/2."""
    assert G_Q[0] == [Fr(-1), 0, 0, 0, 0] and G_Q[7] == [0, 0, 0, 0, Fr(1)]
    assert G_Q[1] == [Fr(-2, 9)] * 5 and G_Q[2] == [Fr(-2, 9) * (-1) ** k for k in range(5)]
    assert G_Q[3] == [Fr(1, 90), Fr(1, 45), Fr(2, 45), Fr(4, 45), Fr(8, 45)]
    assert G_Q[4] == [Fr(1, 90), Fr(-1, 45), Fr(2, 45), Fr(-4, 45), Fr(8, 45)]
    assert G_Q[5] == [Fr(32, 45), Fr(16, 45), Fr(8, 45), Fr(4, 45), Fr(2, 45)]
    assert G_Q[6] == [Fr(32, 45), Fr(-16, 45), Fr(8, 45), Fr(-4, 45), Fr(2, 45)]
    assert BT_Q[0] == [-1, 0, Fr(21, 4), 0, Fr(-21, 4), 0, 1, 0] and AT_Q[3] == [0, 1, -1, 8, -8, Fr(1, 8), Fr(-1, 8), 1]


def _tiles(x):
    """(B, C, T) -> (B, C, T / 4, 8): the frames 4j - 2 .. 4j + 5 of every Winograd tile, zero outside [0, T)."""
    return F.pad(x, (2, 2)).unfold(2, 8, 4)


def _form(x, w, dt):
    """The Winograd form evaluated in dtype dt, the channel sum one channel after the other: (B, M, T)."""
    B, C, T = x.shape
    Uw = torch.einsum("pk,mck->mcp", GM.to(dt), w.to(dt))
    V = torch.einsum("pj,bcnj->bcpn", BT.to(dt), _tiles(x.to(dt)))
    acc = torch.zeros(B, w.shape[0], 8, T // 4, dtype=dt)
    for c in range(C):
        acc = acc + Uw[None, :, c, :, None] * V[:, None, c]
    return torch.einsum("ip,bmpn->bmni", AT.to(dt), acc).reshape(B, w.shape[0], T)


def _scale(x, w):
    """S of the module docstring, fp64."""
    Uw = torch.einsum("pk,mck->mcp", GM, w.double()).abs()
    V = torch.einsum("pj,bcnj->bcpn", BT, _tiles(x.double())).abs()
    return torch.einsum("ip,bmpn->bmni", AT.abs(), torch.einsum("mcp,bcpn->bmpn", Uw, V)).reshape(x.shape[0], w.shape[0], x.shape[2])


def _conv(x, w):
    return F.conv1d(F.pad(x, (2, 2)), w)


def _select(x, ch, tap):
    """out[b][m][t] = x[b][ch[m]][t + tap[m] - 2] (0 outside [0, T)): what a one-hot weight row selects, by indexing."""
    T, xp = x.shape[2], F.pad(x, (2, 2))
    return torch.stack([xp[:, int(c), int(k): int(k) + T] for c, k in zip(ch, tap)], 1)


def _pack_f(w):
    """wp_f[tap][Cin / 16][Cout][16] = w[o][c][tap] (include/glowtts_hip.h)."""
    cout, cin, taps = w.shape
    return w.permute(2, 1, 0).reshape(taps, cin // 16, 16, cout).permute(0, 1, 3, 2).contiguous()


def _case(**kw):
    return types.SimpleNamespace(**kw)


# =============================================================================================== tables and inputs
def _f(B, H, T, why, cond=False, drop=False, ts_null=False):
    return _case(name=f"B{B}-H{H}-T{T}", B=B, H=H, T=T, why=why, cond=cond, drop=drop, ts_null=ts_null)


FWD = [_f(1, 64, 4, "a single tile"),
       _f(3, 64, 4, "every neighbouring lane is another utterance", drop=True),
       _f(2, 64, 8, "two tiles per utterance", cond=True),
       _f(2, 64, 64, "one utterance is one DPP row; ts NULL", ts_null=True),
       _f(3, 64, 68, "51 tiles: a second column group of 3 tiles, row ends inside an utterance", cond=True, drop=True),
       _f(1, 128, 192, "exactly 48 tiles, two row groups", drop=True),
       _f(1, 192, 196, "49 tiles", cond=True),
       _f(5, 64, 36, "utterance ends fall at every lane position", cond=True, drop=True)]


def _b(B, T, why, addend=False, mask=False, y_slice=False, a_strided=False, x_strided=False, lengths=None):
    return _case(name=f"B{B}-T{T}", B=B, T=T, why=why, addend=addend, mask=mask, y_slice=y_slice, a_strided=a_strided,
                 x_strided=x_strided, lengths=lengths or [T] * B)


BWD = [_b(1, 4, "a single tile"),
       _b(3, 4, "every neighbouring lane is another utterance", addend=True, mask=True, y_slice=True, lengths=[4, 1, 3]),
       _b(2, 8, "two tiles per utterance", addend=True, a_strided=True, x_strided=True),
       _b(1, 128, "exactly 32 tiles", addend=True),
       _b(1, 132, "33 tiles", mask=True, lengths=[129]),
       _b(3, 44, "33 tiles across utterances", addend=True, mask=True, y_slice=True, a_strided=True, x_strided=True, lengths=[44, 17, 40]),
       _b(4, 36, "an empty utterance under mask_out", addend=True, mask=True, lengths=[36, 0, 20, 33])]
FWD_PARAMS = [pytest.param(c, id=c.name) for c in FWD]
BWD_PARAMS = [pytest.param(c, id=c.name) for c in BWD]
FILLER_FWD, FILLER_BWD = 16 * 3, 16 * 7          # floats in front of the packed weights in the bound buffer
X_GAP, A_GAP = 8, 12                             # floats between the utterances of a strided x / addend


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def _weights(kind, gen, M, C):
    """(M, C, 5) weights and, for the selection kind, the (channel, tap) of every row."""
    if kind == "random":
        return (torch.randn(M, C, 5, generator=gen, dtype=F64) * (5 * C) ** -0.5).float(), None, None
    ch, tap = torch.randint(0, C, (M,), generator=gen), torch.randint(0, 5, (M,), generator=gen)
    w = torch.zeros(M, C, 5)
    w[torch.arange(M), ch, tap] = 1.0
    return w, ch, tap


def _x(kind, gen, B, C, T):
    if kind == "random":
        return torch.randn(B, C, T, generator=gen) * torch.exp(0.5 * torch.randn(1, C, 1, generator=gen))
    return torch.randint(-8, 9, (B, C, T), generator=gen).float()


@functools.lru_cache(maxsize=None)
def _fwd_inputs(name, kind):
    c = next(c for c in FWD if c.name == name)
    gen = _gen(c.B, c.H, c.T, len(kind))
    I = _case(kind=kind)
    I.x = _x(kind, gen, c.B, c.H, c.T)
    I.w, I.ch, I.tap = _weights(kind, gen, 2 * c.H, c.H)
    I.filler = torch.randn(FILLER_FWD, generator=gen)
    if kind == "random":
        I.bias = 0.1 * torch.randn(2 * c.H, generator=gen)
        I.cond = 0.5 * torch.randn(c.B, 2 * c.H, generator=gen) if c.cond else None
        I.drop_scale = 1.0 / 0.7
    else:
        I.bias = torch.zeros(2 * c.H)
        I.cond = torch.randint(-2, 3, (c.B, 2 * c.H), generator=gen).float() if c.cond else None
        I.drop_scale = 2.0
    I.drop = (torch.rand(c.B, 2 * c.H, c.T, generator=gen) < 0.7).to(torch.uint8) if c.drop else None
    return I


def _gate_from(c, I, pre, s):
    """name -> (value, scale) of the gate on the pre-activation `pre` of conv + bias with operand magnitude s (dtype of pre)."""
    dt = pre.dtype
    if c.drop:
        keep = I.drop.bool()
        pre, s = torch.where(keep, pre * I.drop_scale, torch.zeros_like(pre)), torch.where(keep, s * I.drop_scale, torch.zeros_like(s))
    if c.cond:
        pre, s = pre + I.cond.to(dt)[:, :, None], s + I.cond.to(dt).abs()[:, :, None]
    H = c.H
    th, sg = torch.tanh(pre[:, :H]), torch.sigmoid(pre[:, H:])
    s_th, s_sg = s[:, :H] * (1 - th * th) + (2 + th), s[:, H:] * sg * (1 - sg) + sg         # (tests/test_conv_kernels.py: _gate_ref)
    return {"acts": (th * sg, sg * s_th + th.abs() * s_sg), "th": (th, s_th), "sg": (sg, s_sg)}, pre


@functools.lru_cache(maxsize=None)
def _fwd_want(name, kind):
    """fp64: the gate outputs with their scales, the pre-activation; fp32: the form on the CPU."""
    c, I = next(c for c in FWD if c.name == name), _fwd_inputs(name, kind)
    S = _scale(I.x, I.w) + I.bias.double().abs().view(1, -1, 1)
    pre = (_conv(I.x.double(), I.w.double()) if kind == "random" else _select(I.x.double(), I.ch, I.tap)) + I.bias.double().view(1, -1, 1)
    want, pre = _gate_from(c, I, pre, S)
    cpu, _ = _gate_from(c, I, _form(I.x, I.w, F32) + I.bias.view(1, -1, 1), S.float())
    return want, pre, {k: v[0] for k, v in cpu.items()}


@functools.lru_cache(maxsize=None)
def _bwd_inputs(name, kind):
    c = next(c for c in BWD if c.name == name)
    gen = _gen(c.B, c.T, 3, len(kind))
    I = _case(kind=kind)
    I.x = _x(kind, gen, c.B, C_BWD, c.T)
    I.w, I.ch, I.tap = _weights(kind, gen, M_BWD, C_BWD)
    I.filler = torch.randn(FILLER_BWD, generator=gen)
    r = (lambda *s: torch.randn(*s, generator=gen)) if kind == "random" else (lambda *s: torch.randint(-8, 9, s, generator=gen).float())
    I.addend = r(c.B, M_BWD, c.T) if c.addend else None
    I.x_gap, I.a_gap = torch.randn(c.B, X_GAP, generator=gen), torch.randn(c.B, A_GAP, generator=gen)
    I.mask = (torch.arange(c.T)[None] < torch.tensor(c.lengths)[:, None]).float() if c.mask else None
    return I


def _bwd_finish(c, I, y, s, dt):
    if c.addend:
        y, s = y + I.addend.to(dt), s + I.addend.to(dt).abs()
    if c.mask:
        y, s = y * I.mask.to(dt)[:, None], s * I.mask.to(dt)[:, None]
    return y, s


@functools.lru_cache(maxsize=None)
def _bwd_want(name, kind):
    """(fp64 value, scale, the fp32 form on the CPU)."""
    c, I = next(c for c in BWD if c.name == name), _bwd_inputs(name, kind)
    S = _scale(I.x, I.w)
    y = _conv(I.x.double(), I.w.double()) if kind == "random" else _select(I.x.double(), I.ch, I.tap)
    want, scale = _bwd_finish(c, I, y, S, F64)
    return want, scale, _bwd_finish(c, I, _form(I.x, I.w, F32), S.float(), F32)[0]


def _embed(t, gap):
    """(B, C, T) rows with gap[b] behind utterance b, flat, without the last gap: batch stride C T + gap.shape[1]."""
    B = t.shape[0]
    flat = torch.cat([t.reshape(B, -1), gap], 1).reshape(-1)
    return flat[: flat.numel() - gap.shape[1]]


# =============================================================================================== the library
@pytest.fixture()
def G():
    """The library; restores the arithmetic mode, both bindings, the arming and the two switches afterwards."""
    from glow_tts_train import _hip

    lib = _hip.load()
    before = lib.glowtts_conv_math(-1)
    knobs = {k: _hip.get_knob(k) for k in ("WINO", "WINO_BWD")}
    ns = types.SimpleNamespace(hip=_hip, lib=lib, keep=[], **{k[len("GLOWTTS_PLAN_"):]: v for k, v in _hip.CONSTANTS.items()
                                                             if k.startswith("GLOWTTS_PLAN_")})
    yield ns
    for k, v in knobs.items():
        _hip.set_knob(k, v)
    lib.glowtts_conv_plan_next(None)
    lib.glowtts_conv_bind_planes(None, 0, None)
    lib.glowtts_conv_bind_wino(None, 0, None, 0)
    ns.keep.clear()
    assert lib.glowtts_conv_math(before) == 0


def _u_offset(o):
    """wino_u_offset of csrc/convwino.hip."""
    return ((8 * o + 4) // 5 + 7) // 8 * 8


def _bind_arena(G, D, arena, table_rows):
    """The packed buffer `arena` in a guarded buffer, its U planes made by glowtts_wino_weights for the listed convolutions, both
    plane sets bound to this thread, "bf16x6+wrw" and both switches on -> (pointer of the buffer, plane stride)."""
    n = arena.numel()
    stride = G.hip.wino_plane_elems(n)
    a_ptr = D.inp("arena", arena)
    t_ptr = D.inp("table", torch.tensor(table_rows, dtype=torch.int64))
    u_ptr = D.out("U", (3 * stride,), torch.int16)
    G.hip.call("glowtts_wino_weights", a_ptr, n, t_ptr, len(table_rows), u_ptr, stride)
    planes = torch.empty(3 * n, device="cuda", dtype=torch.int16)
    G.keep.append(planes)
    G.hip.call("glowtts_conv_split_weights", a_ptr, n, planes.data_ptr())
    assert G.lib.glowtts_conv_math(15) == 0
    assert G.lib.glowtts_conv_bind_planes(a_ptr, n, planes.data_ptr()) == 0
    assert G.lib.glowtts_conv_bind_wino(a_ptr, n, u_ptr, stride) == 0
    G.hip.set_knob("WINO", 1)
    G.hip.set_knob("WINO_BWD", 1)
    return a_ptr, stride


def _bf16_to_f64(bits):
    return (bits.to(torch.int32) << 16).view(F32).double()


# =============================================================================================== glowtts_wino_weights
def _slot_channels(nks):
    """channel of [k-step][slot]: chunk lk = slot / 8 holds the channels 4 lk .. 4 lk + 3 of group 2 ks, then of group 2 ks + 1."""
    ks, slot = torch.arange(nks)[:, None], torch.arange(32)[None]
    return 16 * (2 * ks + (slot % 8) // 4) + 4 * (slot // 8) + slot % 4


WEIGHT_CONVS = ((FILLER_FWD, 64, 128), (16 * 5, 384, 192))     # (filler floats in front, Cin, M): a forward and a backward pack


@functools.lru_cache(maxsize=None)
def _weights_arena(kind):
    gen = _gen(17, len(kind))
    parts, convs, off = [], [], 0
    for filler, cin, m in WEIGHT_CONVS:
        w = _weights("random", gen, m, cin)[0] if kind == "random" else torch.randint(-2, 3, (m, cin, 5), generator=gen).float()
        parts += [torch.randn(filler, generator=gen), _pack_f(w).reshape(-1)]
        convs.append(_case(off=off + filler, Cin=cin, M=m, w=w))
        off += filler + w.numel()
    return torch.cat(parts), convs


def _u_want(w):
    """(value, scale) of U[point][k-step][M][32] in fp64."""
    m, cin, _ = w.shape
    ch = _slot_channels(cin // 32)
    val = torch.einsum("pk,mck->pcm", GM, w.double())[:, ch]                  # (8, nks, 32, M)
    sc = torch.einsum("pk,mck->pcm", GM.abs(), w.double().abs())[:, ch]
    return val.permute(0, 1, 3, 2), sc.permute(0, 1, 3, 2)


@gpu
@pytest.mark.parametrize("listed", [(0, 1), (1,)], ids=["both", "one-row"])
def test_wino_weights(G, listed):
    """U planes of the listed convolutions of a buffer that holds two, at offsets that are neither 0 nor multiples of 80: nothing
    outside their ranges is written (the 8-element tail included); the three planes of an element sum exactly to an fp32 value, that
    value is G w to the measured bound and sits at the documented position; integer weights give exactly -w0 and w4 at points 0, 7."""
    for kind in ("random", "int"):
        arena, convs = _weights_arena(kind)
        assert all(c.off % 16 == 0 and c.off % 80 != 0 for c in convs)
        n = arena.numel()
        stride = G.hip.wino_plane_elems(n)
        D = Dev()
        rows = [[convs[i].off, convs[i].Cin // 16, convs[i].M] for i in listed]
        G.hip.call("glowtts_wino_weights", D.inp("arena", arena), n, D.inp("table", torch.tensor(rows, dtype=torch.int64)), len(rows),
                   D.out("U", (3, stride), torch.int16), stride)
        planes = D.finish()["U"]
        untouched = torch.ones(3, stride, dtype=torch.bool)
        figs = []
        for i in listed:
            c = convs[i]
            lo, ne = _u_offset(c.off), 8 * c.Cin * c.M
            assert lo % 8 == 0 and lo + ne + 8 <= stride
            untouched[:, lo: lo + ne] = False
            got = _bf16_to_f64(planes[:, lo: lo + ne]).sum(0).reshape(8, c.Cin // 32, c.M, 32)
            assert torch.equal(got.float().double(), got), "the three planes of an element do not sum to an fp32 value"
            want, scale = _u_want(c.w)
            if kind == "int":
                ch = _slot_channels(c.Cin // 32)
                assert torch.equal(got[0], -c.w.double()[:, ch, 0].permute(1, 0, 2)) and torch.equal(got[7], c.w.double()[:, ch, 4].permute(1, 0, 2))
            fig = units(got, want, scale)
            figs.append(f"Cin {c.Cin} M {c.M} at {c.off}: {fig:.2f} u (bound {BOUNDS['U']})")
            assert fig <= BOUNDS["U"], figs[-1]
        assert bool((planes[untouched] == GUARD[torch.int16]).all()), "written outside the U ranges of the listed convolutions"
        assert int(untouched.sum()) >= 3 * 8
        print(f"wino_weights {kind} {listed}: " + "; ".join(figs))


def test_plane_sizes_never_overlap():
    """glowtts_wino_plane_elems(n) = wino_u_offset(n) + 8, and for the step's buffer (offsets multiples of 16 floats, 5-tap sizes of
    Cin % 32 == 0 and M % 16 == 0, i.e. multiples of 2560 floats): elems(o + n) - elems(o) == 8 n / 5 — the U planes of consecutive
    convolutions have exactly their own size between their starts."""
    from glow_tts_train import _hip

    lib = _hip.load()
    for o in list(range(0, 16 * 400, 16)) + [16 * 12345, 16 * 999999]:
        assert lib.glowtts_wino_plane_elems(o) == _u_offset(o) + 8
        for n in (2560, 2560 * 3, 5 * 64 * 128, 5 * 384 * 192, 2560 * 1001):
            assert lib.glowtts_wino_plane_elems(o + n) - lib.glowtts_wino_plane_elems(o) == 8 * n // 5, (o, n)
    for filler, cin, m in WEIGHT_CONVS:
        assert (5 * cin * m) % 2560 == 0 and filler % 16 == 0


# =============================================================================================== the forward
def _gate_launch(G, c, I):
    """Two launches into two sets of outputs -> (results, launches counted per call)."""
    B, H, T = c.B, c.H, c.T
    D = Dev()
    a_ptr, _ = _bind_arena(G, D, torch.cat([I.filler, _pack_f(I.w).reshape(-1)]), [[FILLER_FWD, H // 16, 2 * H]])
    fixed = [D.inp("x", I.x), a_ptr + 4 * FILLER_FWD, D.inp("bias", I.bias), D.inp("cond", I.cond), D.inp("drop", I.drop), I.drop_scale]
    counted = []
    for rep in ("", "2"):
        before = G.hip.wino_launches()
        G.hip.call("glowtts_conv_gate_fwd", *fixed, D.out("acts" + rep, (B, H, T)), None if c.ts_null else D.out("ts" + rep, (B, 2 * H, T)),
                   B, H, T, 5, 1, 2)
        counted.append(G.hip.wino_launches() - before)
    return D.finish(), counted


def _gate_outputs(c, r, rep=""):
    out = {"acts": r["acts" + rep]}
    if not c.ts_null:
        out["th"], out["sg"] = r["ts" + rep][:, :c.H], r["ts" + rep][:, c.H:]
    return out


def _sel_tolerance_holds(what, values, bound_abs):
    """SEL_TOL is at least the random bound on these inputs and below a quarter of the smallest gap between distinct expected values."""
    v = torch.unique(values)
    gap = float((v[1:] - v[:-1]).min())
    assert v.numel() > 8 and SEL_TOL < gap / 4, (what, gap)
    assert float(bound_abs.max()) <= SEL_TOL, (what, float(bound_abs.max()))


@gpu
@pytest.mark.parametrize("c", FWD_PARAMS)
def test_wino_gate_fwd(G, c):
    """acts and ts of the Winograd kernel, selection and random inputs, the packed weights at a non-zero offset of the bound buffer."""
    for kind in ("select", "random"):
        I = _fwd_inputs(c.name, kind)
        want, pre, _cpu = _fwd_want(c.name, kind)
        r, counted = _gate_launch(G, c, I)
        assert counted == [1, 1], f"{c.name}: the Winograd kernel was launched {counted} times"
        out, figs = _gate_outputs(c, r), []
        for name, g in out.items():
            value, scale = want[name]
            what = f"wino gate {c.name} {kind} {name}"
            assert bool(torch.isfinite(g).all()), what
            assert bits_equal(g, _gate_outputs(c, r, "2")[name]), f"{what}: a second launch gives other bits"
            if kind == "select":
                _sel_tolerance_holds(what, pre, (BOUNDS[name] + SPLIT_EXTRA) * EPS * scale)
                err = (g.double() - value).abs()
                figs.append(f"{name} {float(err.max()):.1e} (tolerance {SEL_TOL:.1e})")
                assert float(err.max()) <= SEL_TOL, f"{what}: off by {float(err.max()):.3e} at {[tuple(i.tolist()) for i in (err > SEL_TOL).nonzero()[:4]]}"
            else:
                fig, bound = units(g, value, scale), BOUNDS[name] + SPLIT_EXTRA
                figs.append(f"{name} {fig:.2f} u (bound {bound})")
                assert fig <= bound, f"{what}: {fig:.2f} u > {bound} u"
        print(f"wino gate {c.name} {kind} [{c.why}]: " + "; ".join(figs))


# =============================================================================================== the backward
def _bwd_buffers(G, c, I, D, reps=("", "2")):
    """Everything of a backward-data launch inside D -> (argument lists per output set, how to read an output set)."""
    B, T = c.B, c.T
    a_ptr, _ = _bind_arena(G, D, torch.cat([I.filler, _pack_f(I.w).reshape(-1)]), [[FILLER_BWD, C_BWD // 16, M_BWD]])
    x_ptr, x_bs = (D.inp("x", _embed(I.x, I.x_gap)), C_BWD * T + X_GAP) if c.x_strided else (D.inp("x", I.x), C_BWD * T)
    a_arg, a_bs = None, 0
    if c.addend:
        a_arg, a_bs = (D.inp("addend", _embed(I.addend, I.a_gap)), M_BWD * T + A_GAP) if c.a_strided else (D.inp("addend", I.addend), M_BWD * T)
    m_ptr = D.inp("mask", I.mask)
    calls = []
    for rep in reps:
        if c.y_slice:                                   # y = the upper channel half of a (B, 2 M, T) tensor
            y_ptr, y_bs = D.out("y" + rep, (B, 2 * M_BWD, T)) + 4 * M_BWD * T, 2 * M_BWD * T
        else:
            y_ptr, y_bs = D.out("y" + rep, (B, M_BWD, T)), M_BWD * T
        calls.append([x_ptr, x_bs, a_ptr + 4 * FILLER_BWD, None, m_ptr, a_arg, a_bs, y_ptr, y_bs, B, C_BWD, M_BWD, T, 5, 1, 2, 0, int(c.mask), 0])

    def read(r, rep=""):
        y = r["y" + rep]
        if c.y_slice:
            assert bool((y[:, :M_BWD] == GUARD[F32]).all()), f"{c.name}: written into the other channel half of y's tensor"
            y = y[:, M_BWD:]
        return y
    return calls, read


def _bwd_check(c, kind, I, y, what, figs):
    want, scale, _cpu = _bwd_want(c.name, kind)
    assert bool(torch.isfinite(y).all()), what
    if c.mask:
        dead = (I.mask == 0)[:, None].expand_as(y)
        assert int(dead.sum()) > 0 and bool((y[dead] == 0).all()), f"{what}: not exactly 0 behind an utterance's end"
    if kind == "select":
        _sel_tolerance_holds(what, _select(I.x.double(), I.ch, I.tap), (BOUNDS["y"] + SPLIT_EXTRA) * EPS * scale)
        err = (y.double() - want).abs()
        figs.append(f"{float(err.max()):.1e} (tolerance {SEL_TOL:.1e})")
        assert float(err.max()) <= SEL_TOL and torch.equal(torch.round(y.double()), want), \
            f"{what}: off by {float(err.max()):.3e} at {[tuple(i.tolist()) for i in (err > SEL_TOL).nonzero()[:4]]}"
    else:
        fig, bound = units(y, want, scale), BOUNDS["y"] + SPLIT_EXTRA
        figs.append(f"{fig:.2f} u (bound {bound})")
        assert fig <= bound, f"{what}: {fig:.2f} u > {bound} u"


@gpu
@pytest.mark.parametrize("c", BWD_PARAMS)
def test_wino_bwd_data(G, c):
    """dx = (conv(x) [+ addend]) [* mask] of the Winograd backward-data kernel, selection and random inputs, strided tensors."""
    for kind in ("select", "random"):
        I = _bwd_inputs(c.name, kind)
        D = Dev()
        calls, read = _bwd_buffers(G, c, I, D)
        counted = []
        for args in calls:
            before = G.hip.wino_bwd_launches()
            G.hip.call("glowtts_conv_fwd", *args)
            counted.append(G.hip.wino_bwd_launches() - before)
        r = D.finish()
        assert counted == [1, 1], f"{c.name}: the Winograd backward-data kernel was launched {counted} times"
        figs = []
        _bwd_check(c, kind, I, read(r), f"wino bwd {c.name} {kind}", figs)
        assert bits_equal(read(r), read(r, "2")), f"wino bwd {c.name} {kind}: a second launch gives other bits"
        print(f"wino bwd {c.name} {kind} [{c.why}]: y " + "; ".join(figs))


@gpu
def test_wino_bwd_workspace_grows_is_reused_and_is_per_stream(G):
    """On a side stream: a small shape, a larger one (the workspace grows), the small one again (the larger workspace is reused), then
    the small one on a second side stream (a workspace of its own); every launch twice: each result is right and the repeat gives the
    same bits, so every arrival counter was back at zero."""
    small, large = next(c for c in BWD if c.name == "B2-T8"), next(c for c in BWD if c.name == "B3-T44")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    figs = []
    for step, (c, stream) in enumerate(((small, s1), (large, s1), (small, s1), (small, s2))):
        I = _bwd_inputs(c.name, "random")
        D = Dev()
        calls, read = _bwd_buffers(G, c, I, D)
        torch.cuda.synchronize()
        before = G.hip.wino_bwd_launches()
        with torch.cuda.stream(stream):
            for args in calls:
                G.hip.call("glowtts_conv_fwd", *args)
        assert G.hip.wino_bwd_launches() - before == 2
        r = D.finish()
        _bwd_check(c, "random", I, read(r), f"wino bwd workspace step {step} {c.name}", figs)
        assert bits_equal(read(r), read(r, "2")), f"step {step}: the repeat gives other bits"
    print("wino bwd workspace (small, large, small, small on a second stream): " + "; ".join(figs))


# =============================================================================================== plans on the CPU
_WP_FLOATS = 1 << 22


@pytest.fixture()
def P(G):
    """G with dummy U planes bound to a dummy packed buffer (a planned call looks at alignment only)."""
    G.wp = 1 << 30
    G.bind = lambda on=True: G.lib.glowtts_conv_bind_wino(G.wp if on else None, _WP_FLOATS if on else 0, (1 << 40) if on else None,
                                                        G.hip.wino_plane_elems(_WP_FLOATS) if on else 0)
    assert G.bind() == 0
    G.hip.set_knob("WINO", 1)
    G.hip.set_knob("WINO_BWD", 1)
    return G


def _plan(P, mode, name, *args):
    assert P.lib.glowtts_conv_math(mode) == 0
    plan = P.hip.ConvPlan()
    assert P.lib.glowtts_conv_plan_next(ctypes.byref(plan)) == 0
    rc = getattr(P.lib, name)(*args, None)
    P.lib.glowtts_conv_plan_next(None)
    assert rc == 0, (name, args, P.lib.glowtts_last_error())
    return plan


_A = lambda i, mis=False: (i << 32) + (4 if mis else 0)          # noqa: E731  (dummy device addresses)


def _gate_plan(P, B, H, T, mode=15, mis=(), drop=True, ts=True, taps=5, dil=1, wp_off=FILLER_FWD):
    return _plan(P, mode, "glowtts_conv_gate_fwd", _A(1, "x" in mis), P.wp + 4 * wp_off, _A(2), _A(3, "cond" in mis),
                 _A(4, "drop" in mis) if drop else None, 2.0, _A(5, "acts" in mis), _A(6, "ts" in mis) if ts else None, B, H, T, taps, dil,
                 (taps - 1) * dil // 2)


def _gate_mirror(B, H, T, mode=15, mis=(), knob=1, bound=True, taps=5, dil=1):
    """plan_wino_gate (csrc/convwino.hip): grid_x, or None where the launch is not the Winograd kernel's."""
    if not knob or (mode & 3) != 3 or not bound or taps != 5 or dil != 1:
        return None
    if H % 64 or T % 4 or set(mis) & {"x", "acts", "ts", "drop"} or B * H * T * 4 >= 0x7ffffff0:
        return None
    return -(-B * (T // 4) // COLS_GATE) * (H // 64)


def _bwd_plan(P, B, T, M=M_BWD, Cin=C_BWD, mode=15, mis=(), bias=False, addend=True, mask_in=0, mask_out=1, mask_add=0, x_gap=0, y_gap=0,
              a_gap=0, taps=5, wp_off=FILLER_BWD):
    return _plan(P, mode, "glowtts_conv_fwd", _A(1, "x" in mis), Cin * T + x_gap, P.wp + 4 * wp_off, _A(2) if bias else None,
                 _A(3, "mask" in mis), _A(4, "addend" in mis) if addend else None, M * T + a_gap, _A(5, "y" in mis), M * T + y_gap, B, Cin, M, T,
                 taps, 1, (taps - 1) // 2, mask_in, mask_out, mask_add)


def _bwd_mirror(B, T, M=M_BWD, Cin=C_BWD, mode=15, mis=(), knob=1, bound=True, bias=False, addend=True, mask_in=0, mask_out=1, mask_add=0,
                x_gap=0, y_gap=0, a_gap=0, taps=5):
    """plan_wino_bwd (csrc/convwino.hip): grid_x, or None."""
    if not knob or (mode & 3) != 3 or not bound or taps != 5 or bias or mask_in or mask_add:
        return None
    if M != 192 or Cin != 2 * M or T % 4:
        return None
    if set(mis) & ({"x", "y"} | ({"addend"} if addend else set()) | ({"mask"} if mask_out else set())):
        return None
    if x_gap % 4 or y_gap % 4 or (addend and a_gap % 4) or B * (Cin * T + x_gap) * 4 >= 0x7ffffff0:
        return None
    return 2 * -(-B * (T // 4) // COLS_BWD)


def _agree(P, plan, grid, family, lds, what):
    if grid is None:
        assert plan.family not in (P.WINO_GATE, P.WINO_BWD), what
    else:
        assert (plan.family, plan.grid_x, plan.grid_y, plan.grid_z, plan.lds_bytes, plan.block, plan.launches) == \
            (family, grid, 1, 1, lds, 256, 1), (what, plan.family, plan.grid_x, plan.lds_bytes)


def test_rows_plan_the_winograd_kernels(P):
    """Every row of the two tables is planned as the kernel it is there for, with the grid and the LDS of the module's constants."""
    for c in FWD:
        plan = _gate_plan(P, c.B, c.H, c.T, drop=c.drop, ts=not c.ts_null)
        tiles = c.B * c.T // 4
        assert (plan.family, plan.lds_bytes, plan.grid_x) == (P.WINO_GATE, LDS_GATE, -(-tiles // COLS_GATE) * (c.H // 64)), c.name
    for c in BWD:
        plan = _bwd_plan(P, c.B, c.T, addend=c.addend, mask_out=int(c.mask), x_gap=X_GAP if c.x_strided else 0,
                         y_gap=M_BWD * c.T if c.y_slice else 0, a_gap=A_GAP if c.a_strided else 0)
        tiles = c.B * c.T // 4
        assert (plan.family, plan.lds_bytes, plan.grid_x) == (P.WINO_BWD, LDS_BWD, 2 * -(-tiles // COLS_BWD)), c.name
    # what the rows are there for
    tiles_f = {c.name: c.B * c.T // 4 for c in FWD}
    assert tiles_f["B3-H64-T68"] == 51 and tiles_f["B1-H128-T192"] == 48 and tiles_f["B1-H192-T196"] == 49
    assert sum(c.T // 4 < 16 for c in FWD) >= 4 and {c.H for c in FWD} == {64, 128, 192}
    assert {(c.cond, c.drop) for c in FWD} == {(False, False), (True, False), (False, True), (True, True)} and any(c.ts_null for c in FWD)
    tiles_b = {c.name: c.B * c.T // 4 for c in BWD}
    assert tiles_b["B1-T128"] == 32 and tiles_b["B1-T132"] == 33 and tiles_b["B3-T44"] == 33
    assert any(0 in c.lengths and c.mask for c in BWD) and {(c.addend, c.mask) for c in BWD} == {(False, False), (True, True), (True, False), (False, True)}
    assert any(c.y_slice for c in BWD) and any(c.a_strided for c in BWD) and any(c.x_strided for c in BWD)
    assert all(c.B <= 17 and c.T <= 200 for c in FWD + BWD)


def test_plans_agree_with_the_mirrors(P):
    """The library's own decisions (glowtts_conv_plan_next: no GPU needed) against the Python restatements of plan_wino_gate and
    plan_wino_bwd over shapes, each alignment bit and each disqualifying flag."""
    n = 0
    for H in range(16, 257, 16):
        for T in range(1, 261):
            for B in range(1, 6):
                _agree(P, _gate_plan(P, B, H, T), _gate_mirror(B, H, T), P.WINO_GATE, LDS_GATE, ("gate", B, H, T))
                n += 1
    for T in range(1, 261):
        for B in range(1, 6):
            _agree(P, _bwd_plan(P, B, T), _bwd_mirror(B, T), P.WINO_BWD, LDS_BWD, ("bwd", B, T))
    for B, H, T in ((3, 64, 68), (1, 192, 196)):
        for mis in ("x", "acts", "ts", "drop", "cond"):
            _agree(P, _gate_plan(P, B, H, T, mis=(mis,)), _gate_mirror(B, H, T, mis=(mis,)), P.WINO_GATE, LDS_GATE, ("gate", mis))
        assert _gate_mirror(B, H, T, mis=("cond",)) is not None and _gate_mirror(B, H, T, mis=("x",)) is None
        for kw in (dict(taps=3), dict(dil=2), dict(mode=0), dict(mode=14), dict(mode=13), dict(mode=3), dict(mode=7)):
            _agree(P, _gate_plan(P, B, H, T, **kw), _gate_mirror(B, H, T, **kw), P.WINO_GATE, LDS_GATE, ("gate", kw))
        assert _gate_mirror(B, H, T, mode=3) is not None and _gate_mirror(B, H, T, mode=14) is None
        P.hip.set_knob("WINO", 0)
        _agree(P, _gate_plan(P, B, H, T), _gate_mirror(B, H, T, knob=0), P.WINO_GATE, LDS_GATE, "gate knob")
        P.hip.set_knob("WINO", 1)
        P.hip.set_knob("WINO_BWD", 0)                   # the backward's switch does not move the forward
        _agree(P, _gate_plan(P, B, H, T), _gate_mirror(B, H, T), P.WINO_GATE, LDS_GATE, "gate, WINO_BWD = 0")
        P.hip.set_knob("WINO_BWD", 1)
        P.bind(False)
        _agree(P, _gate_plan(P, B, H, T), _gate_mirror(B, H, T, bound=False), P.WINO_GATE, LDS_GATE, "gate unbound")
        P.bind()
        _agree(P, _gate_plan(P, B, H, T, wp_off=_WP_FLOATS), _gate_mirror(B, H, T, bound=False), P.WINO_GATE, LDS_GATE, "gate: weights outside the bound buffer")
    for B, T in ((3, 44), (1, 132)):
        variants = [dict(mis=(m,)) for m in ("x", "y", "addend", "mask")] + [dict(mis=("mask",), mask_out=0), dict(mis=("addend",), addend=False)]
        variants += [dict(x_gap=2), dict(y_gap=2), dict(a_gap=2), dict(a_gap=2, addend=False), dict(x_gap=8, y_gap=4, a_gap=12)]
        variants += [dict(bias=True), dict(mask_add=1), dict(mask_in=1), dict(mask_out=0), dict(addend=False), dict(M=128, Cin=256), dict(M=192, Cin=192),
                     dict(M=64, Cin=128), dict(taps=3), dict(mode=0), dict(mode=14), dict(mode=3)]
        for kw in variants:
            _agree(P, _bwd_plan(P, B, T, **kw), _bwd_mirror(B, T, **kw), P.WINO_BWD, LDS_BWD, ("bwd", B, T, kw))
        assert _bwd_mirror(B, T, mis=("mask",), mask_out=0) is not None and _bwd_mirror(B, T, a_gap=2, addend=False) is not None
        assert _bwd_mirror(B, T, x_gap=8, y_gap=4, a_gap=12) is not None and _bwd_mirror(B, T, bias=True) is None
        P.hip.set_knob("WINO_BWD", 0)
        _agree(P, _bwd_plan(P, B, T), _bwd_mirror(B, T, knob=0), P.WINO_BWD, LDS_BWD, "bwd knob")
        P.hip.set_knob("WINO_BWD", 1)
        P.hip.set_knob("WINO", 0)                       # the forward's switch does not move the backward
        _agree(P, _bwd_plan(P, B, T), _bwd_mirror(B, T), P.WINO_BWD, LDS_BWD, "bwd, WINO = 0")
        P.hip.set_knob("WINO", 1)
        P.bind(False)
        _agree(P, _bwd_plan(P, B, T), _bwd_mirror(B, T, bound=False), P.WINO_BWD, LDS_BWD, "bwd unbound")
        P.bind()
    assert n == 16 * 260 * 5
    assert 2 * 3 * 8 * COLS_GATE * 16 * 4 == LDS_GATE and 2 * 3 * 8 * COLS_BWD * 16 * 4 == LDS_BWD     # two images [3][8][columns][16 dwords]


# =============================================================================================== the bound table on the CPU
def _fp32_cpu_figures():
    """key -> the worst figure of the form in fp32 torch on the CPU against fp64 over the tables (the 'fp32 CPU' column)."""
    figs = {k: 0.0 for k in BOUNDS}
    for c in FWD:
        want, _pre, cpu = _fwd_want(c.name, "random")
        for name, (value, scale) in want.items():
            figs[name] = max(figs[name], units(cpu[name], value, scale))
    for c in BWD:
        want, scale, cpu = _bwd_want(c.name, "random")
        figs["y"] = max(figs["y"], units(cpu, want, scale))
    for conv in _weights_arena("random")[1]:
        want, scale = _u_want(conv.w)
        cpu = torch.einsum("pk,mck->pcm", GM.float(), conv.w)[:, _slot_channels(conv.Cin // 32)].permute(0, 1, 3, 2)
        figs["U"] = max(figs["U"], units(cpu, want, scale))
    return figs


def test_bound_table_matches_fp32_cpu_evaluation():
    """Every bound is 4 x the fp32-CPU figure rounded up to a power of two: fig <= bound <= 16 fig (4 x, the rounding to a power of
    two, and a factor 2 for another CPU's vector width)."""
    figs = _fp32_cpu_figures()
    for key, fig in sorted(figs.items()):
        print(f"fp32 CPU {key}: {fig:.2f} u (bound {BOUNDS[key]}, on the GPU + {SPLIT_EXTRA if key != 'U' else 0})")
    for key, fig in figs.items():
        bound = BOUNDS[key]
        assert bound == 2 ** round(math.log2(bound)), key
        assert fig <= bound <= 16 * fig, (key, fig, bound)


def test_selection_inputs_on_the_cpu():
    """On the selection inputs the fp32 form itself stays far inside SEL_TOL, the random bound does too, and distinct expected values
    are whole numbers apart: the tolerance tells a selected value from any other."""
    worst = 0.0
    for c in FWD:
        I = _fwd_inputs(c.name, "select")
        want, pre, cpu = _fwd_want(c.name, "select")
        assert torch.equal(pre, torch.round(pre))
        for name, (value, scale) in want.items():
            _sel_tolerance_holds((c.name, name), pre, (BOUNDS[name] + SPLIT_EXTRA) * EPS * scale)
            worst = max(worst, float((cpu[name].double() - value).abs().max()))
        sel = _select(I.x.double(), I.ch, I.tap)
        assert torch.equal(sel, _conv(I.x.double(), I.w.double()))
    for c in BWD:
        I = _bwd_inputs(c.name, "select")
        want, scale, cpu = _bwd_want(c.name, "select")
        assert torch.equal(want, torch.round(want))
        _sel_tolerance_holds(c.name, _select(I.x.double(), I.ch, I.tap), (BOUNDS["y"] + SPLIT_EXTRA) * EPS * scale)
        worst = max(worst, float((cpu.double() - want).abs().max()))
    print(f"selection inputs: the fp32 form on the CPU deviates by at most {worst:.1e} (tolerance {SEL_TOL:.1e})")
    assert worst <= SEL_TOL / 8
