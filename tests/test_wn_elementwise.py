"""The element-wise kernels of csrc/wn.hip one by one, through the C ABI (glow_tts_train._hip.call), against plain torch on the CPU:
gate_fwd, gate_bwd, gate_bwd_ts, res_skip_fwd, res_skip_bwd and res_skip_bwd_io (fp32 and bf16 tensors).  The training path
reaches them only where the fused convolution kernels do not apply, and the parity tests see them through whole WN stacks at
rtol 2e-4.  The GPU tests are marked `gpu`; the test at the end of the module checks the bound table on the CPU.

Every launch (_Dev, as in tests/test_flow_kernels.py): each input is a copy inside a guarded buffer and must be bit-identical
afterwards; each output lives between guard sentinels that must survive and is pre-filled with the sentinel.  Inputs beyond an
utterance's end hold random finite values; from two utterances on, one has length 0.

Shapes (B, H, T), each launcher being ceil(B H T / width / 256) workgroups of the 16-byte (width 4) or the scalar kernels:
    (2, 8, 7)    T % 4 != 0: the scalar kernels
    (3, 8, 36)   the vector kernels; then each tensor of the launcher's alignment test in turn one float off a 16-byte boundary:
                 the scalar kernels
    (1, 4, 300)  300 vector items: a second, partial workgroup

res_skip_fwd / _bwd / _bwd_io: every output element is one addition and one multiplication by a 0/1 mask, or a copy (for bf16
tensors: a bf16 value times 0 or 1): asserted EQUAL to fp32 torch on the CPU, bf16 tensors bit for bit.  `last` 0 and 1, with and
without skip_in / dx, io 0 and 1.

gate_fwd / _bwd (with and without the conditioning row g) / _bwd_ts (with and without keep bytes): against fp64, per element in
units of u = 2**-24 times the magnitude of the operands, with the scales tests/test_conv_kernels.py uses for the same formulas
(S_pre = |a| + |g|; S_tanh = S_pre (1 - tanh^2) + 2 + tanh; S_sigmoid = S_pre sigmoid (1 - sigmoid) + sigmoid).  Each bound is 4 x
what plain fp32 torch on the CPU shows against fp64 on the same inputs (worst over the three shapes), rounded up to a power of two:
    output                    scale                                                                    fp32 CPU   bound   MI355X
    gate_fwd acts             sigmoid S_tanh + |tanh| S_sigmoid                                        0.90 u      4 u   0.90 u
    gate_bwd da               |dacts| sigmoid (1 + tanh^2) ; |dacts| |tanh| sigmoid (1 + sigmoid)      3.38 u     16 u   4.12 u
    gate_bwd_ts da            the same from the stored tanh / sigmoid, times the keep scale            2.74 u     16 u   2.74 u
(gate_bwd recomputes tanh and sigmoid from a + g, so its figure carries their rounding; gate_bwd_ts reads them.)
test_bound_table_matches_fp32_cpu_evaluation recomputes the column and asserts fig <= bound <= 16 fig.
Counting inputs (small integers; stored tanh in {-1/2, 0, 1/2}, sigmoid in {1/4, 1/2, 3/4}, keep scale 2): gate_bwd_ts is exact in
fp32 and asserted EQUAL; where a pre-activation is exactly 0 the gate must give (acts, tanh, sigmoid) = (0, 0, 1/2) exactly: acts
== 0 from gate_fwd, and from gate_bwd da = (dacts / 2, 0) where both pre-activations of an element are 0.
"""
import functools
import math
import types

import pytest
import torch

gpu = pytest.mark.gpu

U = 2.0 ** -24
GUARD = {torch.float32: -1234.5, torch.bfloat16: -1232.0, torch.uint8: 165}
INT_OF = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.uint8: torch.uint8}
PAD_BYTES = 32           # guard on each side: the payload stays 16-byte aligned

BOUNDS = {"acts": 4, "da": 16, "da_ts": 16}          # in u: the table of the module docstring

SHAPES = [((2, 8, 7), "T % 4 != 0: the scalar kernels"),
          ((3, 8, 36), "the vector kernels; then each tensor in turn one float off a 16-byte boundary: the scalar kernels"),
          ((1, 4, 300), "300 vector items: a second, partial workgroup")]
SHAPE_PARAMS = [pytest.param(s, id="x".join(map(str, s))) for s, _why in SHAPES]

# the tensors of each launcher's alignment test (can_vec4)
VEC_TENSORS = {"gate_fwd": ("a", "acts"), "gate_bwd": ("a", "dacts", "da"), "gate_bwd_ts": ("ts", "dacts", "da"),
               "res_skip_fwd": ("x", "rs", "mask", "skip_in", "x_out", "skip_out"),
               "res_skip_bwd": ("dx_out", "dskip", "mask", "dx", "drs")}


@pytest.fixture(scope="module")
def G():
    from glow_tts_train import _hip

    _hip.load()
    return types.SimpleNamespace(hip=_hip)


def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(INT_OF[a.dtype]), b.contiguous().view(INT_OF[b.dtype]))


def _units(got, want, scale):
    """max over elements of |got - want| / (u * scale); where the scale is 0 the values must agree exactly."""
    got, want, scale = got.detach().cpu().double().reshape(-1), want.detach().double().reshape(-1), scale.detach().double().reshape(-1)
    err = (got - want).abs()
    zero = scale == 0
    assert bool((err[zero] == 0).all()), "difference where the operands are all zero"
    if bool(zero.all()):
        return 0.0
    return float((err[~zero] / (U * scale[~zero])).max())


class _Dev:
    """The buffers of one raw-ABI call: inputs are copies inside guarded buffers (bit-identical afterwards), outputs live between
    guard sentinels.  `mis` names the one tensor that starts one float (4 bytes) off a 16-byte boundary."""

    def __init__(self, mis=None):
        self.mis, self.ins, self.outs, self.seen = mis, [], [], set()

    def _place(self, name, numel, dtype):
        esz = torch.empty(0, dtype=dtype).element_size()
        pad, off = PAD_BYTES // esz, (4 // esz if name == self.mis else 0)
        self.seen.add(name)
        buf = torch.full((numel + 2 * pad,), GUARD[dtype], dtype=dtype, device="cuda")
        view = buf[pad + off: pad + off + numel]
        assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == esz * off
        return buf, view, pad + off

    def inp(self, name, t):
        if t is None:
            return None
        buf, view, lo = self._place(name, t.numel(), t.dtype)
        view.copy_(t.reshape(-1))
        self.ins.append((name, t, buf, lo))
        return view.data_ptr()

    def out(self, name, shape, dtype=torch.float32):
        numel = int(math.prod(shape))
        buf, view, lo = self._place(name, numel, dtype)
        self.outs.append((name, shape, buf, lo, numel))
        return view.data_ptr()

    def finish(self):
        torch.cuda.synchronize()
        assert self.mis is None or self.mis in self.seen, self.mis
        for name, t, buf, lo in self.ins:
            b, hi = buf.cpu(), lo + t.numel()
            assert _bits_equal(b[lo:hi], t.reshape(-1)), f"input {name} changed"
            assert bool((b[:lo] == GUARD[t.dtype]).all()) and bool((b[hi:] == GUARD[t.dtype]).all()), f"written around input {name}"
        res = {}
        for name, shape, buf, lo, numel in self.outs:
            b, hi = buf.cpu(), lo + numel
            assert bool((b[:lo] == GUARD[b.dtype]).all()) and bool((b[hi:] == GUARD[b.dtype]).all()), f"guard of output {name} overwritten"
            res[name] = b[lo:hi].reshape(shape).clone()
        return res


# =============================================================================================== inputs
@functools.lru_cache(maxsize=8)
def _inputs(kind, B, H, T):
    """Everything any kernel of the module reads, fp32 on the CPU."""
    gen = torch.Generator().manual_seed(7919 * B + 104729 * H + T + len(kind))
    I = types.SimpleNamespace(kind=kind, B=B, H=H, T=T)
    lengths = torch.randint(1, T + 1, (B,), generator=gen)
    lengths[0] = T if B >= 2 else max(1, T - 3)
    if B >= 2:
        lengths[B // 2] = 0                                   # one utterance of length 0
    I.lengths = lengths
    I.mask = (torch.arange(T)[None] < lengths[:, None]).float()
    rn = lambda *shape: torch.randn(shape, generator=gen)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=gen).float()
    if kind == "count":
        I.a, I.g, I.dacts = ri(-1, 1, B, 2 * H, T), ri(-1, 1, B, 2 * H), ri(-2, 2, B, H, T)
        I.ts = torch.cat([ri(-1, 1, B, H, T) / 2, ri(1, 3, B, H, T) / 4], 1)
        I.drop_scale = 2.0
    else:
        I.a, I.g, I.dacts = rn(B, 2 * H, T), rn(B, 2 * H), rn(B, H, T)
        I.ts = torch.cat([torch.tanh(rn(B, H, T).double()).float(), torch.sigmoid(rn(B, H, T).double()).float()], 1)
        I.drop_scale = 1.0 / 0.7
    I.drop = (torch.rand(B, 2 * H, T, generator=gen) < 0.7).to(torch.uint8)
    I.x, I.rs, I.skip, I.dx_out, I.dskip = rn(B, H, T), rn(B, 2 * H, T), rn(B, H, T), rn(B, H, T), rn(B, H, T)
    return I


# =============================================================================================== references
def _gate_ref(op, I, dt, cond=True, drop=True):
    """(value, scale) of acts (gate_fwd) or da (gate_bwd, gate_bwd_ts) in dtype dt with plain torch on the CPU."""
    H = I.H
    go = I.dacts.to(dt)
    if op == "gate_bwd_ts":
        th, sg = I.ts[:, :H].to(dt), I.ts[:, H:].to(dt)
    else:
        a = I.a.to(dt)
        g = I.g.to(dt)[:, :, None] if cond else torch.zeros(I.B, 2 * H, 1, dtype=dt)
        pre, s_pre = a + g, a.abs() + g.abs()
        th, sg = torch.tanh(pre[:, :H]), torch.sigmoid(pre[:, H:])
        if op == "gate_fwd":
            # the operands of the last operation of tanh = 2 / (1 + e^-2x) - 1 are 1 + tanh and 1; sigmoid is a quotient
            s_th, s_sg = s_pre[:, :H] * (1 - th * th) + (2 + th), s_pre[:, H:] * sg * (1 - sg) + sg
            return th * sg, sg * s_th + th.abs() * s_sg
    # 1 - th^2 and 1 - sg are differences of 1 and a value below 1: their operands are 1 + th^2 and 1 + sg
    v = torch.cat([go * sg * (1 - th * th), go * th * sg * (1 - sg)], 1)
    s = torch.cat([go.abs() * sg * (1 + th * th), go.abs() * th.abs() * sg * (1 + sg)], 1)
    if op == "gate_bwd_ts" and drop:
        keep = I.drop.bool()
        v, s = torch.where(keep, v * I.drop_scale, torch.zeros_like(v)), torch.where(keep, s * I.drop_scale, torch.zeros_like(s))
    return v, s


def _res_skip_fwd_ref(I, last, with_skip):
    """fp32 torch on the CPU: (x_out or None, skip_out)."""
    H, m = I.H, I.mask[:, None]
    sk = I.skip if with_skip else torch.zeros(I.B, H, I.T)
    if last:
        return None, (sk + I.rs[:, :H]) * m                   # rs is (B, H, T)
    return (I.x + I.rs[:, :H]) * m, sk + I.rs[:, H:]


def _res_skip_bwd_ref(dx_out, dskip, mask, last):
    """(dx or None, drs) in the tensors' own dtype: the arithmetic is fp32, a value times 0 or 1 rounds back unchanged."""
    m = mask[:, None]
    if last:
        return None, (dskip.float() * m).to(dskip.dtype)
    gx = (dx_out.float() * m).to(dx_out.dtype)
    return gx, torch.cat([gx, dskip], 1)


# =============================================================================================== the launches
def _launch_gate(G, op, I, cond=True, drop=True, mis=None):
    D = _Dev(mis)
    B, H, T = I.B, I.H, I.T
    g = D.inp("g", I.g) if cond else None
    if op == "gate_fwd":
        G.hip.call("glowtts_gate_fwd", D.inp("a", I.a), g, D.out("acts", (B, H, T)), B, H, T)
        return D.finish()["acts"]
    if op == "gate_bwd":
        G.hip.call("glowtts_gate_bwd", D.inp("a", I.a), g, D.inp("dacts", I.dacts), D.out("da", (B, 2 * H, T)), B, H, T)
    else:
        G.hip.call("glowtts_gate_bwd_ts", D.inp("ts", I.ts), D.inp("dacts", I.dacts), D.inp("drop", I.drop) if drop else None,
                   I.drop_scale if drop else 1.0, D.out("da", (B, 2 * H, T)), B, H, T)
    return D.finish()["da"]


def _misalignments(op, shape):
    return [None] + (list(VEC_TENSORS[op]) if shape == (3, 8, 36) else [])


def _check_gate(what, key, got, want, scale):
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
    fig = _units(got, want, scale)
    print(f"{what}: {fig:.2f} u (bound {BOUNDS[key]})")
    assert fig <= BOUNDS[key], f"{what}: {fig:.2f} u > {BOUNDS[key]} u"


# =============================================================================================== 1. the gate
@gpu
@pytest.mark.parametrize("shape", SHAPE_PARAMS)
def test_gate_fwd(G, shape):
    """acts = tanh(a[:, :H] + g) sigmoid(a[:, H:] + g), with and without g; counting inputs: acts == 0 exactly wherever the
    tanh half's pre-activation is 0."""
    for cond in (True, False):
        for mis in _misalignments("gate_fwd", shape):
            I = _inputs("random", *shape)
            want, scale = _gate_ref("gate_fwd", I, torch.float64, cond=cond)
            _check_gate(f"gate_fwd {shape} g={int(cond)} misaligned={mis}", "acts", _launch_gate(G, "gate_fwd", I, cond=cond, mis=mis), want, scale)
        I = _inputs("count", *shape)
        got = _launch_gate(G, "gate_fwd", I, cond=cond)
        zero = (I.a + (I.g[:, :, None] if cond else 0))[:, :I.H] == 0
        assert int(zero.sum()) >= shape[0] * shape[2] and bool((got[zero] == 0).all()), "tanh(0) sigmoid(.) has to be exactly 0"
        want, scale = _gate_ref("gate_fwd", I, torch.float64, cond=cond)
        _check_gate(f"gate_fwd {shape} g={int(cond)} count", "acts", got, want, scale)


@gpu
@pytest.mark.parametrize("shape", SHAPE_PARAMS)
def test_gate_bwd(G, shape):
    """da from (a, g, dacts), the activations recomputed; counting inputs: where both pre-activations of an element are exactly 0,
    tanh = 0 and sigmoid = 1/2 exactly: da = (dacts / 2, 0)."""
    for cond in (True, False):
        for mis in _misalignments("gate_bwd", shape):
            I = _inputs("random", *shape)
            want, scale = _gate_ref("gate_bwd", I, torch.float64, cond=cond)
            _check_gate(f"gate_bwd {shape} g={int(cond)} misaligned={mis}", "da", _launch_gate(G, "gate_bwd", I, cond=cond, mis=mis), want, scale)
        I, H = _inputs("count", *shape), shape[1]
        got = _launch_gate(G, "gate_bwd", I, cond=cond)
        pre = I.a + (I.g[:, :, None] if cond else 0)
        both = (pre[:, :H] == 0) & (pre[:, H:] == 0)
        assert int(both.sum()) >= 8
        assert torch.equal(got[:, :H][both], I.dacts[both] / 2) and bool((got[:, H:][both] == 0).all()), "(tanh, sigmoid)(0) != (0, 1/2)"
        assert bool((got[:, H:][pre[:, :H] == 0] == 0).all())


@gpu
@pytest.mark.parametrize("shape", SHAPE_PARAMS)
def test_gate_bwd_ts(G, shape):
    """da from the stored tanh / sigmoid, with and without the forward's keep bytes and scale; counting inputs: EQUAL."""
    for drop in (True, False):
        for mis in _misalignments("gate_bwd_ts", shape):
            I = _inputs("random", *shape)
            want, scale = _gate_ref("gate_bwd_ts", I, torch.float64, drop=drop)
            got = _launch_gate(G, "gate_bwd_ts", I, drop=drop, mis=mis)
            _check_gate(f"gate_bwd_ts {shape} drop={int(drop)} misaligned={mis}", "da_ts", got, want, scale)
            if drop:
                assert bool((got[I.drop == 0] == 0).all()), "a dropped element has gradient 0"
        I = _inputs("count", *shape)
        want, scale = _gate_ref("gate_bwd_ts", I, torch.float64, drop=drop)
        assert float(scale.max()) * 64 < 2 ** 24              # sixty-fourths of small integers: exact in fp32
        got = _launch_gate(G, "gate_bwd_ts", I, drop=drop)
        assert torch.equal(got.double(), want), f"gate_bwd_ts {shape} count drop={int(drop)}: differs from exact arithmetic"


# =============================================================================================== 2. residual / skip
@gpu
@pytest.mark.parametrize("shape", SHAPE_PARAMS)
def test_res_skip_fwd(G, shape):
    """x_out = (x + rs[:, :H]) mask, skip_out = skip_in + rs[:, H:]; last: skip_out = (skip_in + rs) mask and x_out is left alone
    (given or not); skip_in may be NULL.  EQUAL to fp32 torch."""
    B, H, T = shape
    I = _inputs("random", *shape)
    for last, with_skip, with_x in [(0, True, True), (0, False, True), (1, True, False), (1, False, False), (1, True, True)]:
        want_x, want_skip = _res_skip_fwd_ref(I, last, with_skip)
        for mis in _misalignments("res_skip_fwd", shape):
            if (mis == "skip_in" and not with_skip) or (mis in ("x", "x_out") and not with_x):
                continue
            D = _Dev(mis)
            rs = I.rs[:, :H].contiguous() if last else I.rs
            G.hip.call("glowtts_res_skip_fwd", D.inp("x", I.x) if with_x else None, D.inp("rs", rs), D.inp("mask", I.mask),
                       D.inp("skip_in", I.skip) if with_skip else None, D.out("x_out", (B, H, T)) if with_x else None,
                       D.out("skip_out", (B, H, T)), B, H, T, last)
            got = D.finish()
            what = f"res_skip_fwd {shape} last={last} skip_in={int(with_skip)} x={int(with_x)} misaligned={mis}"
            assert torch.equal(got["skip_out"], want_skip), what
            if last:
                assert not with_x or bool((got["x_out"] == GUARD[torch.float32]).all()), what + ": x_out written"
            else:
                assert torch.equal(got["x_out"], want_x), what
            assert bool((got["skip_out"][I.lengths == 0] == 0).all()) or not last
            print(what + ": ==")


@gpu
@pytest.mark.parametrize("io", [0, 1], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPE_PARAMS)
def test_res_skip_bwd(G, shape, io):
    """drs = [dx_out mask ; dskip] and dx = dx_out mask (dx may be NULL); last: drs = dskip mask.  glowtts_res_skip_bwd_io with fp32
    (io = 0) and bf16 (io = 1) tensors, and the fp32 entry point glowtts_res_skip_bwd: EQUAL to torch, bf16 bit for bit."""
    B, H, T = shape
    I = _inputs("random", *shape)
    dt = torch.bfloat16 if io else torch.float32
    dx_out, dskip = I.dx_out.to(dt), I.dskip.to(dt)
    for last, with_dx in [(0, True), (0, False), (1, False), (1, True)]:
        want_dx, want_drs = _res_skip_bwd_ref(dx_out, dskip, I.mask, last)
        for entry in (("glowtts_res_skip_bwd_io",) if io else ("glowtts_res_skip_bwd_io", "glowtts_res_skip_bwd")):
            for mis in _misalignments("res_skip_bwd", shape):
                if (mis == "dx" and not with_dx) or (mis == "dx_out" and last and not with_dx):
                    continue
                D = _Dev(mis)
                args = [D.inp("dx_out", dx_out) if (not last or with_dx) else None, D.inp("dskip", dskip), D.inp("mask", I.mask),
                        D.out("dx", (B, H, T), dt) if with_dx else None, D.out("drs", (B, H if last else 2 * H, T), dt), B, H, T, last]
                G.hip.call(entry, *args, *((io,) if entry.endswith("_io") else ()))
                got = D.finish()
                what = f"{entry} {shape} io={io} last={last} dx={int(with_dx)} misaligned={mis}"
                assert _bits_equal(got["drs"], want_drs) if io else torch.equal(got["drs"], want_drs), what
                if with_dx and not last:
                    assert _bits_equal(got["dx"], want_dx) if io else torch.equal(got["dx"], want_dx), what
                if with_dx and last:
                    assert bool((got["dx"] == GUARD[dt]).all()), what + ": dx written"
                print(what + ": ==")


# =============================================================================================== 3. the bound table, on the CPU
def test_bound_table_matches_fp32_cpu_evaluation():
    """Every bound is 4 x the figure of plain fp32 torch on the CPU against fp64 (worst over SHAPES, with and without g / keep
    bytes), rounded up to a power of two: fig <= bound <= 16 fig."""
    figs = {}
    for (shape, _why) in SHAPES:
        I = _inputs("random", *shape)
        for key, op, kws in (("acts", "gate_fwd", ({"cond": True}, {"cond": False})), ("da", "gate_bwd", ({"cond": True}, {"cond": False})),
                             ("da_ts", "gate_bwd_ts", ({"drop": True}, {"drop": False}))):
            for kw in kws:
                want, scale = _gate_ref(op, I, torch.float64, **kw)
                got, _ = _gate_ref(op, I, torch.float32, **kw)
                figs[key] = max(figs.get(key, 0.0), _units(got, want, scale))
    for key, fig in sorted(figs.items()):
        print(f"fp32 CPU {key}: {fig:.2f} u (bound {BOUNDS[key]})")
    assert set(figs) == set(BOUNDS)
    for key, fig in figs.items():
        bound = BOUNDS[key]
        assert bound == 2 ** round(math.log2(bound)), key
        assert fig <= bound <= 16 * fig, (key, fig, bound)


def test_counting_gate_bwd_ts_is_exact_in_fp32_on_the_cpu():
    for (shape, _why) in SHAPES:
        I = _inputs("count", *shape)
        for drop in (True, False):
            assert torch.equal(_gate_ref("gate_bwd_ts", I, torch.float32, drop=drop)[0].double(), _gate_ref("gate_bwd_ts", I, torch.float64, drop=drop)[0])
