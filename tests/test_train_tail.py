"""GPU tests (-m gpu) of the small kernels the training step ends in (csrc/train_ops.hip), one by one against fp64 on the CPU:
mle_fwd / mle_finish / mle_bwd, dur_fwd / dur_bwd, span_logw, squeeze / unsqueeze, adam / adam_advance.  Every gradient and every
parameter update passes through them; the end-to-end tests only reach them where their mistakes cancel (one Adam update from zero
moments is lr * sign(g) whatever the betas are; one element dropped from a sum of 1e6 moves the loss by 1e-6 of itself).

References are plain torch / numpy in fp64: oracle.mle_loss, duration_loss, squeeze, unsqueeze, noam_lr, and torch.optim.Adam on
fp64 CPU tensors.  Where a kernel receives a hyper-parameter as a C float, the reference uses that fp32 value (see _f32).

Where each bound comes from (u = 2**-24, half a unit in the last place of an fp32 number in [1, 2)):
  * reductions, random inputs: |got - want| <= 1e-5 * sum|term_i| / denominator — the project's own figure for this reduction
    structure (block sum + one atomic per workgroup, <= 512 workgroups), tests/test_grad_accum.py::test_clip_grad_value_scaled_vs_torch.
    fp32 torch on the CPU against fp64 gives 2e-8 .. 4e-8 in these units at the shapes used here;
  * reductions, counting inputs (terms 0, 0.5, 2; 0/1 masks; every partial sum an integer multiple of 0.5 far below 2**24, hence
    exact in fp32 in ANY order): the sums and counts are asserted EQUAL to integer arithmetic, the loss to one fp32 rounding
    (rel <= 2**-23) of the exact quotient — a dropped or double-counted element, a wrong tail, a wrong mask count show at any size;
  * element-wise outputs: per element, in units of u times the magnitude of the operands of the last operation (so cancellation
    cannot hide in a relative tolerance); the bound is 4 x what the fp32 CPU evaluation of the same formula shows against fp64
    (the reference alone), rounded up to a power of two:
        output      scale                         fp32 CPU, these inputs    bound
        dz          |dz|                          3.9 u                     16 u
        dlogs       sc (1 + e d^2)                4.6 u                     16 u
        dlogw       |dlogw|                       1.9 u                      8 u
        span_logw   1 + |log(1e-8 + count)|       0.9 u                      4 u
        Adam m      |b1 m| + |(1 - b1) g|         1.9 u                      8 u
        Adam v      |v|                           2.6 u                     16 u
        Adam p      |p| + |update|                6.7 u (torch), 9.2 u *    32 u
    (* the kernel's own sequence of fp32 operations evaluated with numpy on the CPU.  The Adam p figure depends on the base rate:
    an error of a few u of |b1 m| + |(1 - b1) g| in m is a large RELATIVE error of m where the two cancel, and the scale
    |p| + |update| does not see it once the step is large against |p| — with a base rate of 0.75 fp32 torch itself is 110 u off
    on these moments; the test uses 0.01, where the imposed rate 0.0241 gives the largest steps.)  The figures each test prints
    are the MI355X's; none may exceed its bound;
  * data movement (squeeze / unsqueeze, guards, untouched inputs, the zero padding of the flat buffers): exact equality.
"""
import functools
import math
import types

import numpy as np
import pytest
import torch

from helpers import assert_close

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
DLOSS = 0.37
GUARD = -1234.5          # sentinel in front of and behind every raw-ABI output


def _f32(x):
    """The value a C `float` argument of the ABI holds.  The fp64 references use it: 1 - fl(0.98) differs from 0.02 by 9.5e-7
    relative — a property of the interface, not a rounding of the kernel."""
    return float(np.float32(x))


@pytest.fixture(scope="module")
def G():
    from glow_tts_train import _hip, ops, optimize, utils
    from oracle import glow_oracle as O

    _hip.load()
    return types.SimpleNamespace(hip=_hip, ops=ops, optimize=optimize, utils=utils, O=O)


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


# =============================================================================================== 1. mle_loss
MLE_SHAPES = [(1, 1, 1),            # a single element
              (2, 5, 7),            # n % 4 != 0: the scalar kernel
              (3, 80, 37),          # vector kernel, partial last workgroup
              (2, 80, 4000),        # nv = 160000: the second unrolled half partly in range
              (5, 80, 3001),        # nv = 300100: a second loop iteration whose second half is out of range
              (1, 83, 3163),        # odd n = 262529 > 2 * 131072 on the scalar kernel
              (300, 4, 8)]          # B > 256: the batch loops of the finish kernel and of the dlogdet fill


def _mle_inputs(B, C, T, kind, seed):
    gen = torch.Generator().manual_seed(seed)
    mask = _mask(_ragged(gen, B, T), T)
    if kind == "count":       # logs = 0, z - m in {0, +-1, +-2}: every term is 0, 0.5 or 2; -logdet a small non-negative integer
        m = torch.randint(-3, 4, (B, C, T), generator=gen).float()
        d = torch.randint(-2, 3, (B, C, T), generator=gen)
        z, logs = m + d.float(), torch.zeros(B, C, T)
        logdet = -torch.randint(0, 4, (B,), generator=gen).float()
        return z, m, logs, logdet, mask, d
    z = torch.randn(B, C, T, generator=gen)
    m = 0.5 * torch.randn(B, C, T, generator=gen)
    logs = 0.3 * torch.randn(B, C, T, generator=gen)
    logdet = 0.1 * C * T * torch.randn(B, generator=gen)
    return z, m, logs, logdet, mask, None


def _mle_exact(d, logdet, mask, C):
    """Integer arithmetic: (sum of the terms, sum of the mask, denominator, loss in fp64)."""
    acc0 = int((d.long() ** 2).sum()) / 2.0
    acc1 = int(mask.long().sum())
    denom = acc1 * C
    num = acc0 - int(logdet.long().sum())
    assert 2 * acc0 < 2 ** 24 and denom < 2 ** 24 and num >= 0
    return acc0, acc1, denom, num / denom + 0.5 * math.log(2 * math.pi)


def _mle_loss_fwd_raw(G, z, m, logs, mask, logdet):
    B, C, T = z.shape
    acc = torch.zeros(2, device="cuda")
    out = torch.full((2,), GUARD, device="cuda")
    G.hip.call("glowtts_mle_loss_fwd", z.data_ptr(), m.data_ptr(), logs.data_ptr(), mask.data_ptr(), logdet.data_ptr(),
               acc.data_ptr(), out.data_ptr(), B, C, T)
    return acc.cpu(), out.cpu()


@pytest.mark.parametrize("shape", MLE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mle_counting_inputs_are_exact(G, shape):
    B, C, T = shape
    z, m, logs, logdet, mask, d = _mle_inputs(B, C, T, "count", seed=B * C * T)
    acc0, acc1, denom, loss = _mle_exact(d, logdet, mask, C)
    acc, out = _mle_loss_fwd_raw(G, *(t.cuda() for t in (z, m, logs, mask, logdet)))
    rel = abs(float(out[0]) - loss) / loss
    print(f"mle counting {shape}: acc {acc.tolist()} want [{acc0}, {acc1}]; denom {float(out[1])} want {denom}; "
          f"loss rel err {rel:.2e} (bound {2.0 ** -23:.2e})")
    assert float(acc[0]) == acc0 and float(acc[1]) == acc1, (acc.tolist(), acc0, acc1)
    assert float(out[1]) == denom
    assert rel <= 2.0 ** -23


@pytest.mark.parametrize("shape", MLE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mle_random_vs_fp64(G, shape):
    """ops.MleLossFn forward and backward (dloss = 0.37) against autograd through oracle.mle_loss in fp64.
    fp32 torch on the CPU, same inputs, worst over the shapes: loss 5.6e-8 of sum|term| / denom (bound 1e-5), dz 3.9 u (bound 16 u),
    dlogs 4.6 u (bound 16 u)."""
    B, C, T = shape
    z, m, logs, logdet, mask, _ = _mle_inputs(B, C, T, "random", seed=1 + B * C * T)
    dl = _f32(DLOSS)
    # ---- fp64 reference
    z64, m64, l64, ld64 = (t.double().requires_grad_(True) for t in (z, m, logs, logdet))
    want = G.O.mle_loss(z64, m64, l64, ld64, mask.double()[:, None])
    want.backward(torch.tensor(dl, dtype=torch.float64))
    denom = float(mask.sum()) * C
    e, d = torch.exp(-2 * l64.detach()), (z64 - m64).detach()
    cond = float((l64.detach() + 0.5 * e * d * d).abs().sum() + ld64.detach().abs().sum()) / denom
    # ---- the kernels
    zg, mg, lg, ldg = (t.cuda().requires_grad_(True) for t in (z, m, logs, logdet))
    loss = G.ops.MleLossFn.apply(zg, mg, lg, ldg, mask.cuda())
    loss.backward(torch.tensor(DLOSS, device="cuda"))
    fig = abs(float(loss.detach()) - float(want.detach())) / cond
    sc = dl / denom
    u_dz = _units(zg.grad, z64.grad, z64.grad.abs())
    u_dl = _units(lg.grad, l64.grad, sc * (1 + e * d * d))
    print(f"mle random {shape}: loss {float(loss.detach()):.7f} want {float(want.detach()):.7f}, |err| / (sum|term| / denom) = {fig:.2e} (bound 1e-5); "
          f"dz {u_dz:.2f} u (bound 16), dlogs {u_dl:.2f} u (bound 16)")
    assert fig <= 1e-5
    assert u_dz <= 16 and u_dl <= 16
    assert _bits_equal(mg.grad, -zg.grad)                                   # dm == -dz bit for bit
    dld = ldg.grad.cpu()
    assert dld.shape == (B,) and bool((dld == dld[0]).all())                # every b, the same value
    assert abs(float(dld[0]) + sc) <= 2.0 ** -23 * sc                       # == -dloss / denom to one rounding
    # the same launch into buffers that held a sentinel: every element of every output is written, with the same bits
    outs = [torch.full_like(zg, GUARD) for _ in range(3)] + [torch.full((B,), GUARD, device="cuda")]
    dloss, den = torch.tensor([DLOSS], device="cuda"), torch.tensor([denom], device="cuda")
    G.hip.call("glowtts_mle_loss_bwd", zg.data_ptr(), mg.data_ptr(), lg.data_ptr(), dloss.data_ptr(), den.data_ptr(),
               *(o.data_ptr() for o in outs), B, B * C * T)
    assert all(_bits_equal(a, b.grad) for a, b in zip(outs, (zg, mg, lg, ldg)))


def test_mle_raw_abi_misaligned_pointers(G):
    """n % 4 == 0 but every pointer one element off a 16-byte boundary: the scalar kernel has to be taken, and it computes what the
    vector kernel computes on aligned buffers.  Every output sits between guard elements."""
    B, C, T = 3, 80, 37
    n = B * C * T
    assert n % 4 == 0

    def place(t, off):
        """A copy of `t` at element `off` of a guarded buffer: (buffer, view)."""
        buf = torch.full((t.numel() + PAD,), GUARD, device="cuda")
        view = buf[off: off + t.numel()]
        view.copy_(t.reshape(-1))
        assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4 * off
        return buf, view

    def guards_intact(buf, off, size):
        return bool((buf[:off] == GUARD).all()) and bool((buf[off + size:] == GUARD).all())

    # ---- forward, counting inputs: both kernels give the integer answer
    z, m, logs, logdet, mask, d = _mle_inputs(B, C, T, "count", seed=77)
    acc0, acc1, _, _ = _mle_exact(d, logdet, mask, C)
    maskg = mask.cuda()
    for off in (0, 1):
        ins = [place(t, off)[1] for t in (z, m, logs)]
        acc = torch.zeros(2, device="cuda")
        G.hip.call("glowtts_mle_fwd", ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), maskg.data_ptr(), acc.data_ptr(), B, C, T)
        assert acc.tolist() == [acc0, float(acc1)], (off, acc.tolist(), acc0, acc1)

    # ---- forward and backward, random inputs
    z, m, logs, logdet, mask, _ = _mle_inputs(B, C, T, "random", seed=78)
    maskg = mask.cuda()
    denom = float(mask.sum()) * C
    l64 = logs.double()
    e, dd = torch.exp(-2 * l64), z.double() - m.double()
    terms = l64 + 0.5 * e * dd * dd
    sc = _f32(DLOSS) / denom
    dloss, den = torch.tensor([DLOSS], device="cuda"), torch.tensor([denom], device="cuda")
    results = {}
    for off in (0, 1):
        ins = [place(t, off)[1] for t in (z, m, logs)]
        before = [t.clone() for t in ins]
        acc = torch.zeros(2, device="cuda")
        G.hip.call("glowtts_mle_fwd", ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), maskg.data_ptr(), acc.data_ptr(), B, C, T)
        fig = abs(float(acc[0]) - float(terms.sum())) / float(terms.abs().sum())
        print(f"mle_fwd raw, pointer offset {off}: |acc0 - want| / sum|term| = {fig:.2e} (bound 1e-5)")
        assert fig <= 1e-5 and float(acc[1]) == float(mask.sum())
        bufs, outs = zip(*[place(torch.full((n,), GUARD), off) for _ in range(3)])
        dldbuf, dld = place(torch.full((B,), GUARD), off)
        G.hip.call("glowtts_mle_loss_bwd", ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), dloss.data_ptr(), den.data_ptr(),
                   outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), dld.data_ptr(), B, n)
        assert all(torch.equal(a, b) for a, b in zip(ins, before))          # inputs untouched
        assert all(guards_intact(buf, off, n) for buf in bufs) and guards_intact(dldbuf, off, B)
        u_dz = _units(outs[0], sc * e * dd, (sc * e * dd).abs())
        u_dl = _units(outs[2], sc * (1 - e * dd * dd), sc * (1 + e * dd * dd))
        print(f"mle_loss_bwd raw, pointer offset {off}: dz {u_dz:.2f} u (bound 16), dlogs {u_dl:.2f} u (bound 16)")
        assert u_dz <= 16 and u_dl <= 16
        assert _bits_equal(outs[1], -outs[0])
        assert bool((dld == dld[0]).all()) and abs(float(dld[0]) + sc) <= 2.0 ** -23 * sc
        # glowtts_mle_bwd (the scale handed over ready-made) is the same arithmetic
        bufs2, outs2 = zip(*[place(torch.full((n,), GUARD), off) for _ in range(3)])
        scale = (-dld[:1]).clone()
        G.hip.call("glowtts_mle_bwd", ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), scale.data_ptr(),
                   outs2[0].data_ptr(), outs2[1].data_ptr(), outs2[2].data_ptr(), n)
        assert all(_bits_equal(a, b) for a, b in zip(outs2, outs))
        assert all(guards_intact(buf, off, n) for buf in bufs2)
        results[off] = [o.clone() for o in outs] + [dld.clone()]
    assert all(_bits_equal(a, b) for a, b in zip(results[0], results[1]))   # scalar and vector kernel: the same answer


# =============================================================================================== 2. duration loss
DUR_SHAPES = [(1, 1), (3, 37), (32, 160), (300, 5), (64, 513)]


def _dur_inputs(B, Tx, kind, seed):
    gen = torch.Generator().manual_seed(seed)
    lengths = _ragged(gen, B, Tx).long()
    if kind == "count":
        logw_ = torch.randint(0, 6, (B, 1, Tx), generator=gen).float()
        d = torch.randint(-2, 3, (B, 1, Tx), generator=gen)
        return logw_ + d.float(), logw_, lengths, d
    logw_ = torch.randint(1, 40, (B, 1, Tx), generator=gen).float().log()          # log of a token's frame count
    return logw_ + 0.5 * torch.randn(B, 1, Tx, generator=gen), logw_, lengths, None


@pytest.mark.parametrize("shape", DUR_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_duration_loss_counting_inputs_are_exact(G, shape):
    B, Tx = shape
    logw, logw_, lengths, d = _dur_inputs(B, Tx, "count", seed=B * Tx)
    s, l = int((d.long() ** 2).sum()), int(lengths.sum())
    assert 0 < l and s < 2 ** 24
    lw, lw_, lg = logw.cuda(), logw_.cuda(), lengths.cuda()
    out = torch.full((2,), GUARD, device="cuda")
    G.hip.call("glowtts_duration_loss_fwd", lw.data_ptr(), lw_.data_ptr(), lg.data_ptr(), out.data_ptr(), B, B * Tx)
    rel = abs(float(out[0]) - s / l) / max(s / l, 1e-300)
    print(f"duration counting {shape}: denominator {float(out[1])} want {l}; loss {float(out[0])!r} want {s / l!r}, rel err {rel:.2e} "
          f"(bound {2.0 ** -23:.2e})")
    assert float(out[1]) == l
    assert rel <= 2.0 ** -23
    assert float(G.ops.DurationLossFn.apply(lw, lw_, lg)) == float(out[0])         # the wrapper launches the same thing


@pytest.mark.parametrize("shape", DUR_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_duration_loss_random_vs_fp64(G, shape):
    """ops.DurationLossFn forward and backward (dloss = 0.37) against oracle.duration_loss and 2 (logw - logw_) dloss / sum(lengths).
    fp32 torch on the CPU, same inputs, worst over the shapes: loss 2.8e-8 of itself (every term is positive; bound 1e-5),
    dlogw 1.9 u (bound 8 u = 4 x 1.9 rounded up to a power of two)."""
    B, Tx = shape
    logw, logw_, lengths, _ = _dur_inputs(B, Tx, "random", seed=1 + B * Tx)
    dl = _f32(DLOSS)
    want = G.O.duration_loss(logw.double(), logw_.double(), lengths)
    dwant = 2 * (logw.double() - logw_.double()) * dl / float(lengths.sum())
    lw, lw_ = logw.cuda().requires_grad_(True), logw_.cuda().requires_grad_(True)
    loss = G.ops.DurationLossFn.apply(lw, lw_, lengths.cuda())
    loss.backward(torch.tensor(DLOSS, device="cuda"))
    fig = abs(float(loss.detach()) - float(want)) / float(want)                      # sum|term| / denom is the loss itself
    u_d = _units(lw.grad, dwant, dwant.abs())
    print(f"duration random {shape}: loss {float(loss.detach()):.7f} want {float(want):.7f}, |err| / (sum|term| / denom) = {fig:.2e} (bound 1e-5); "
          f"dlogw {u_d:.2f} u (bound 8)")
    assert fig <= 1e-5
    assert lw.grad.shape == logw.shape and u_d <= 8
    assert lw_.grad is None                                                 # the alignment is a constant of the step


# =============================================================================================== 3. span_logw
def _span_table(B, Tx, seed):
    """Cumulative sums of random span lengths (0, 1, a few frames, up to 4000), ragged t_x with a 0 and a full row; what lies
    behind a row's t_x is rubbish that would give NaN if it were read into the result."""
    gen = torch.Generator().manual_seed(seed)
    kind = torch.rand(B, Tx, generator=gen)
    span = torch.randint(2, 60, (B, Tx), generator=gen)
    span = torch.where(kind < 0.2, torch.zeros_like(span), span)
    span = torch.where((kind >= 0.2) & (kind < 0.4), torch.ones_like(span), span)
    span = torch.where(kind >= 0.9, torch.randint(60, 4001, (B, Tx), generator=gen), span)
    forced = torch.tensor([4000, 0, 1])[:Tx]
    span[0, : forced.numel()] = forced
    t_x = _ragged(gen, B, Tx)
    first = torch.zeros(B, Tx + 1, dtype=torch.int64)
    first[:, 1:] = span.cumsum(1)
    behind = torch.arange(Tx + 1)[None] > t_x[:, None]
    first[behind] = -7
    assert int(first.max()) < 2 ** 31
    return first.int(), t_x.int()


def _span_want(first, t_x):
    count = (first[:, 1:].long() - first[:, :-1].long()).double()
    live = torch.arange(count.shape[1])[None] < t_x[:, None]
    want = torch.where(live, torch.log(1e-8 + count.clamp_min(0)), torch.zeros_like(count))
    return want[:, None], live[:, None]


def _check_span(G, first, t_x, what):
    want, live = _span_want(first, t_x)
    got = G.ops.span_logw(first.cuda(), t_x.cuda()).cpu()
    assert got.shape == want.shape and got.dtype == torch.float32
    assert bool((got[~live] == 0.0).all())                                  # exactly 0 behind t_x
    fig = _units(got, want, 1 + want.abs())
    print(f"span_logw {what}: {fig:.2f} u of 1 + |log| (bound 4)")
    assert fig <= 4


@pytest.mark.parametrize("shape", [(1, 1), (3, 37), (7, 160), (520, 1009)], ids=lambda s: "x".join(map(str, s)))
def test_span_logw_synthetic(G, shape):
    """(520, 1009): B * Tx > 2048 * 256, the grid-stride loop.  The scale 1 + |log|: one rounding of the argument (1e-8 + count) moves
    the logarithm by up to u, the logarithm's own rounding by up to u |log|.  fp32 torch on the CPU: 0.9 u (bound 4 u)."""
    B, Tx = shape
    first, t_x = _span_table(B, Tx, seed=B + Tx)
    if Tx >= 3:
        counts = (first[0, 1:4] - first[0, :3]).tolist()
        assert counts == [4000, 0, 1]
    _check_span(G, first, t_x, str(shape))


def test_span_logw_of_a_searched_alignment(G):
    B, Tx, Ty = 4, 37, 101
    gen = torch.Generator().manual_seed(5)
    value = torch.randn(B, Tx, Ty, generator=gen)
    t_x = torch.tensor([37, 20, 1, 9])
    t_y = torch.tensor([101, 77, 13, 9])
    path, first, _tok = G.ops.mas_path_spans(value.cuda(), t_x.cuda(), t_y.cuda())
    path = path.cpu().double()
    live = (torch.arange(Tx)[None] < t_x[:, None])[:, None]
    assert float(path.sum()) == float(t_y.sum())                            # one token per frame
    want = torch.log(1e-8 + path.sum(-1))[:, None] * live
    got = G.ops.span_logw(first, t_x.cuda()).cpu()
    assert bool((got[~live] == 0.0).all())
    fig = _units(got, want, 1 + want.abs())
    print(f"span_logw of mas_path_spans ({B}, {Tx}, {Ty}): {fig:.2f} u of 1 + |log| (bound 4)")
    assert fig <= 4


# =============================================================================================== 4. squeeze / unsqueeze
SQZ_C = (1, 6, 80)


def _sqz_mask(gen, B, T):
    lengths = torch.randint(1, T + 1, (B,), generator=gen)
    lengths[0], lengths[1] = T, max(1, T - 3)
    return _mask(lengths, T)[:, None]


@pytest.mark.parametrize("io", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("T", [11, 12, 37])
@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_squeeze_forward_backward_roundtrip(G, n, T, io):
    """utils.squeeze, its backward and the round trip through utils.unsqueeze against autograd through oracle.squeeze / unsqueeze:
    the kernels move data and multiply by a 0/1 mask, so rtol = atol = 0 (bf16: the fp32 result converted with .to(bfloat16))."""
    B, Ts = 3, T // n
    dt = torch.bfloat16 if io else torch.float32
    for C in SQZ_C:
        gen = torch.Generator().manual_seed(1000 * n + 10 * T + C)
        x = torch.randn(B, C, T, generator=gen)
        mask = _sqz_mask(gen, B, T)
        w = torch.randn(B, C * n, Ts, generator=gen).to(dt)                 # the gradient arriving at the squeezed tensor
        # ---- oracle
        xr = x.clone().requires_grad_(True)
        xs_ref, ms_ref = G.O.squeeze(xr, mask, n)
        xs_ref.backward(w.float())
        back_ref, mo_ref = G.O.unsqueeze(xs_ref.detach().to(dt).float(), ms_ref, n)
        # ---- kernels
        xg = x.cuda().requires_grad_(True)
        xs, ms = G.utils.squeeze(xg, mask.cuda(), n, io_bf16=io)
        assert xs.dtype == dt and xs.shape == (B, C * n, Ts) and ms.shape == (B, 1, Ts)
        what = f"n={n} T={T} C={C} io={io}"
        assert_close(xs.float(), xs_ref.detach().to(dt).float(), rtol=0, atol=0, what="squeeze " + what)
        assert_close(ms, ms_ref, rtol=0, atol=0, what="squeezed mask " + what)
        xs.backward(w.cuda())
        assert_close(xg.grad, xr.grad, rtol=0, atol=0, what="squeeze backward " + what)
        assert bool((xg.grad[:, :, Ts * n:] == 0).all())                    # frames cut off by the floor division
        back, mo = G.utils.unsqueeze(xs.detach(), ms, n, io_bf16=io)
        assert back.dtype == torch.float32 and back.shape == (B, C, Ts * n)
        assert_close(back, back_ref, rtol=0, atol=0, what="round trip " + what)
        assert_close(mo, mo_ref, rtol=0, atol=0, what="round trip mask " + what)
        keep = mask[:, :, n - 1::n].repeat_interleave(n, dim=2)
        assert_close(back, (x[:, :, : Ts * n] * keep).to(dt).float() if io else x[:, :, : Ts * n] * keep, rtol=0, atol=0,
                     what="round trip is x * mask " + what)


@pytest.mark.parametrize("io", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("T", [11, 12, 37])
@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_unsqueeze_forward_backward(G, n, T, io):
    B, Ts = 3, T // n
    dt = torch.bfloat16 if io else torch.float32
    for C in SQZ_C:
        gen = torch.Generator().manual_seed(2000 * n + 10 * T + C)
        xs = torch.randn(B, C * n, Ts, generator=gen).to(dt)
        ms = _sqz_mask(gen, B, Ts)
        w = torch.randn(B, C, Ts * n, generator=gen)                        # the gradient arriving at the un-squeezed tensor
        xr = xs.float().clone().requires_grad_(True)                        # a leaf of its own: .float() of fp32 is xs itself
        x_ref, mo_ref = G.O.unsqueeze(xr, ms, n)
        x_ref.backward(w)
        xg = xs.cuda().requires_grad_(True)
        x, mo = G.utils.unsqueeze(xg, ms.cuda(), n, io_bf16=io)
        what = f"n={n} T={T} C={C} io={io}"
        assert x.dtype == torch.float32 and x.shape == (B, C, Ts * n) and mo.shape == (B, 1, Ts * n)
        assert_close(x, x_ref.detach(), rtol=0, atol=0, what="unsqueeze " + what)
        assert_close(mo, mo_ref, rtol=0, atol=0, what="unsqueezed mask " + what)
        x.backward(w.cuda())
        assert xg.grad.dtype == dt
        assert_close(xg.grad.float(), xr.grad.to(dt).float(), rtol=0, atol=0, what="unsqueeze backward " + what)


# =============================================================================================== 5. Adam / Noam
LR, DIM = 0.01, 192.0
ADAM_STATES = [(1.0, 1.0, 0.0), (4.0, 2.0, 0.0241), (100000.0, 100000.0, 0.0), (7.0, 123456.0, 0.0)]      # (t, s, imposed rate)
ADAM_HYPER = [(0.9, 0.98, 1e-9), (0.9, 0.999, 1e-8)]
PAD = 8


@functools.lru_cache(maxsize=None)
def _adam_data(n):
    """(p, g, m, v) of n + PAD floats each, on the CPU.  |g| log-uniform in [1e-6, 10] with random sign, a share of exact zeros;
    m ~ 0.1 N, v ~ 0.1 U; a share of elements with g = m = v = 0 (what the padding of the flat buffers holds)."""
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
    return p, g, m, v, dead


def _adam_ref(G, p, g, m, v, state, lr, b1, b2, eps, dim, warmup):
    """One torch.optim.Adam update (no amsgrad, no weight decay) in fp64; the rate as optimize.py:32-48 sets it."""
    t, s, imposed = state
    rate = imposed if imposed > 0 else (lr if warmup <= 0 else G.O.noam_lr(s, dim, warmup, lr))
    m1 = b1 * m + (1 - b1) * g
    v1 = b2 * v + (1 - b2) * g * g
    upd = rate / (1 - b1 ** t) * (m1 / (v1.sqrt() / math.sqrt(1 - b2 ** t) + eps))
    return p - upd, m1, v1, upd


@pytest.mark.parametrize("state", ADAM_STATES, ids=lambda s: "t%g-s%g-lr%g" % s)
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "off1"])
@pytest.mark.parametrize("n", [1, 5, 1023, 4099, 600001, 2 ** 21 + 4])
def test_adam_one_update_raw(G, n, offset, state):
    """glowtts_adam_noam on buffers the test fills itself, non-trivial moments, against fp64.
    On the CPU, same inputs, worst over all cases: torch's fp32 operations m 1.8 u, v 2.0 u, p 6.7 u; the kernel's sequence of fp32
    operations in numpy m 1.9 u, v 2.6 u, p 9.2 u (bounds 8 u, 16 u, 32 u)."""
    cpu = _adam_data(n)
    dead = cpu[4][offset: offset + n]
    p64, g64, m64, v64 = (t[offset: offset + n].double() for t in cpu[:4])
    base = [t.cuda() for t in cpu[:4]]
    assert all(t.data_ptr() % 16 == 0 for t in base)
    st0 = torch.tensor([state[0], state[1], 123.0, state[2]], dtype=torch.float32)
    worst = [0.0, 0.0, 0.0]
    for warmup in (4000.0, 0.0):
        for b1, b2, eps in ADAM_HYPER:
            bufs = [t.clone() for t in base]
            p, g, m, v = (t[offset: offset + n] for t in bufs)
            assert (p.data_ptr() % 16 == 0) == (offset == 0)
            st = st0.cuda()
            G.hip.call("glowtts_adam_noam", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, st.data_ptr(),
                       LR, b1, b2, eps, DIM, warmup)
            # the reference sees the hyper-parameters as the fp32 values the ABI receives (_f32), the state as the fp32 it is
            f1, f2, fe = _f32(b1), _f32(b2), _f32(eps)
            want_p, want_m, want_v, upd = _adam_ref(G, p64, g64, m64, v64, tuple(float(x) for x in st0[[0, 1, 3]]),
                                                    _f32(LR), f1, f2, fe, DIM, warmup)
            figs = [_units(m, want_m, (f1 * m64).abs() + ((1 - f1) * g64).abs()),
                    _units(v, want_v, want_v.abs()),
                    _units(p, want_p, p64.abs() + upd.abs())]
            worst = [max(a, b) for a, b in zip(worst, figs)]
            assert figs[0] <= 8 and figs[1] <= 16 and figs[2] <= 32, (warmup, b1, b2, eps, figs)
            assert torch.equal(st.cpu(), st0)                                           # state and gradient unchanged
            assert _bits_equal(bufs[1], base[1])
            for buf, b0 in zip(bufs, base):                                             # nothing outside [offset, offset + n)
                assert _bits_equal(buf[:offset], b0[:offset]) and _bits_equal(buf[offset + n:], b0[offset + n:])
            # g == m == v == 0: p bit for bit, moments stay zero — what keeps the flat buffers' padding at zero
            dg = dead.cuda()
            assert _bits_equal(p[dg], base[0][offset: offset + n][dg])
            assert bool((m[dg] == 0).all()) and bool((v[dg] == 0).all())
    if n >= 5:
        assert bool(dead.any()) and not bool(dead.all())
    print(f"adam n={n} offset={offset} state={state}: m {worst[0]:.2f} u (bound 8), v {worst[1]:.2f} u (bound 16), "
          f"p {worst[2]:.2f} u (bound 32)")


def _noam_f32(s, lr, dim, warmup):
    """optimize.py:32-41 in numpy fp64, rounded to fp32."""
    s, w = np.float64(s), np.float64(warmup)
    return np.float32(np.float64(lr) * np.power(np.float64(dim), -0.5) * np.min([np.power(s, -0.5), s * np.power(w, -1.5)]))


@pytest.mark.parametrize("s1", [2, 3999, 4000, 4001, 100000, 2 ** 24 - 1])
def test_adam_advance(G, s1):
    lr = 0.1
    for warmup in (4000.0, 0.0):
        for t in (1.0, float(s1 - 1), 7.0):
            st = torch.tensor([t, float(s1 - 1), 123.0, 0.5], device="cuda")
            G.hip.call("glowtts_adam_advance", st.data_ptr(), lr, DIM, warmup)
            got = st.cpu().numpy()
            assert got[0] == np.float32(t + 1) and got[1] == np.float32(s1) and got[3] == 0.0, got
            if warmup <= 0:
                assert got[2] == np.float32(lr), got
            else:
                want = float(_noam_f32(s1, _f32(lr), DIM, warmup))
                rel = abs(float(got[2]) - want) / want
                print(f"adam_advance s+1={s1} t={t:g}: rate {float(got[2])!r} want {want!r} rel {rel:.2e} (bound {2.0 ** -23:.2e})")
                assert rel <= 2.0 ** -23


def _trajectory(G, scheduler, updates, lr, seed):
    """`updates` updates of three parameters (1, 65 and 4099 elements: the flat layout pads between them) through optimize.Adam,
    each with its own seeded gradient, against torch.optim.Adam on fp64 CPU copies whose rate is set to noam_lr(k) before
    update k (optimize.py:43-55).  e_ref — the same updates by torch.optim.Adam in fp32 on the CPU against the fp64 run — is the
    reference's own error and sets the bound: per tensor max|p - p64| <= max(4 e_ref, 16 u max|p|)."""
    sizes, dim, warm = (1, 65, 4099), 192, 10
    b1, b2, eps = _f32(0.9), _f32(0.98), _f32(1e-9)
    gen = torch.Generator().manual_seed(seed)
    init = [torch.randn(n, generator=gen) for n in sizes]
    params = [torch.nn.Parameter(t.clone().cuda()) for t in init]
    opt = G.optimize.Adam(params, scheduler=scheduler, dim_model=dim, warmup_steps=warm, lr=lr, betas=(b1, b2), eps=eps)
    flat = opt._optim
    pad = torch.ones(flat.numel_padded, dtype=torch.bool)
    for o, n in flat.slices():
        pad[o: o + n] = False
    assert int(pad.sum()) == flat.numel_padded - sum(sizes) > 0
    pad = pad.cuda()
    p64 = [t.double().requires_grad_(True) for t in init]
    p32 = [t.clone().requires_grad_(True) for t in init]
    ref64 = torch.optim.Adam(p64, lr=lr, betas=(b1, b2), eps=eps)
    ref32 = torch.optim.Adam(p32, lr=lr, betas=(b1, b2), eps=eps)
    assert float(flat.dev_state[0]) == 1.0 and float(flat.dev_state[1]) == 1.0
    for k in range(1, updates + 1):
        rate = G.O.noam_lr(k, dim, warm, lr) if scheduler == "noam" else lr
        assert abs(opt.cur_lr - rate) <= 1e-12 * rate                      # the host mirror is the reference's schedule
        for ref in (ref64, ref32):
            ref.param_groups[0]["lr"] = rate
        for i, n in enumerate(sizes):
            g = torch.randn(n, generator=gen)
            g = torch.where(g >= 0, g + 1e-3, g - 1e-3)                     # |g| >= 1e-3
            params[i].grad.copy_(g)
            p64[i].grad, p32[i].grad = g.double(), g.clone()
        opt.step()
        ref64.step()
        ref32.step()
        st = flat.dev_state.cpu()
        assert float(st[0]) == k + 1 and float(st[1]) == k + 1 and float(st[3]) == 0.0, (k, st)
        assert abs(float(st[2]) - opt.cur_lr) <= 2.0 ** -23 * opt.cur_lr, (k, float(st[2]), opt.cur_lr)
        for buf in (flat.flat_p, flat.flat_m, flat.flat_v):
            assert bool((buf[pad] == 0).all()), k
        sd = opt.state_dict()["state"]
        assert all(float(sd[i]["step"]) == k for i in range(len(sizes)))
    for i, n in enumerate(sizes):
        want = p64[i].detach()
        e_ref = float((p32[i].detach().double() - want).abs().max())
        err = float((params[i].detach().cpu().double() - want).abs().max())
        bound = max(4 * e_ref, 16 * U * float(want.abs().max()))
        print(f"adam trajectory scheduler={scheduler} {updates} updates, {n} elements: max|p - p64| = {err:.3e}, fp32 CPU torch "
              f"e_ref = {e_ref:.3e}, bound {bound:.3e}")
        assert err <= bound, (n, err, e_ref, bound)


def test_adam_trajectory_noam_vs_torch_fp64(G):
    """fp32 torch on the CPU ends 1e-7 .. 1e-6 from the fp64 run (e_ref, measured in the test and printed); the kernel's sequence of
    fp32 operations, evaluated with numpy on the CPU, lands on the same figures to two digits."""
    _trajectory(G, "noam", 30, 1.0, seed=11)


def test_adam_trajectory_constant_rate_vs_torch_fp64(G):
    _trajectory(G, None, 5, _f32(0.01), seed=12)
