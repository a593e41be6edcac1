"""GPU parity tests (-m gpu): the HIP path, called through the C ABI (libglowtts_hip.so via ctypes), against
  (1) golden vectors produced by the real reference (tests/golden, oracle/make_golden.py),
  (2) the CPU oracle (oracle/) on seeded inputs at sizes it finishes in seconds,
  (3) size-independent properties at BASELINE.json's full sizes (flow invertibility, MAS path structure).

Tolerances: MAS bit-exact; fp32 kernels 1e-3 relative (BASELINE.json north_star) — most checks are far tighter and
say so.
"""
import os

import numpy as np
import pytest
import torch

from helpers import T, assert_close, load_golden, rel_err, split_prefix

pytestmark = pytest.mark.gpu

REL = 1e-3          # north-star tolerance
TIGHT = dict(rtol=1e-4, atol=2e-5)


@pytest.fixture(scope="module")
def G():
    """The drop-in package (fails loudly if the HIP library is absent)."""
    from glow_tts_train import _hip, attentions, layers, models, monotonic_align, ops, optimize, utils

    _hip.load()

    class NS:
        pass

    ns = NS()
    ns.hip, ns.attentions, ns.layers, ns.models = _hip, attentions, layers, models
    ns.mas, ns.ops, ns.optimize, ns.utils = monotonic_align, ops, optimize, utils
    return ns


@pytest.fixture(params=["fp32", "bf16x6+wrw"])
def conv_mode(request):
    """Arithmetic of the WN-stack convolutions for the tests that exercise them against the reference's vectors / the
    oracle: native fp32 MFMA and the fp32-equivalent bf16-plane form (csrc/convgemm_split.hip), SAME tolerances — so the
    driver's own `pytest -m gpu` run covers both."""
    from glow_tts_train import convops

    before = convops.set_conv_math(request.param)
    yield request.param
    convops.set_conv_math(before)


def dev(a, **kw):
    return T(a, **kw).cuda()


def load_sd(module, golden, prefix="sd."):
    sd = split_prefix(golden, prefix)
    module.load_state_dict(sd)
    return module.cuda()


def check_param_grads(module, golden, what, rtol=2e-4, atol=5e-5):
    gg = split_prefix(golden, "grad.")
    named = dict(module.named_parameters())
    assert gg
    for k, want in gg.items():
        assert named[k].grad is not None, f"{what}: no grad for {k}"
        assert_close(named[k].grad, want, what=f"{what} grad {k}", rtol=rtol, atol=atol)


# =============================================================================================== library
def test_library_is_the_hip_one(G):
    lib = G.hip.load()
    assert lib.glowtts_abi_version() == 1
    assert G.hip.library_path().endswith("glow-tts-train_amd/lib/libglowtts_hip.so")
    with pytest.raises(RuntimeError):
        G.ops.mask_len(torch.ones(2, 3))          # CPU tensor: no fallback, loud failure
    with pytest.raises(RuntimeError, match="n_split"):
        x = torch.zeros(1, 12, 4, device="cuda")
        G.ops.invconv_apply(x, torch.ones(1, 4, device="cuda"), torch.eye(3, device="cuda"), 3)      # odd: layers.py:227


# =============================================================================================== MAS
@pytest.fixture(params=[1, 0], ids=["multiwave", "singlewave"])
def mas_kernel(request, G):
    """Both forms of the search (csrc/mas.hip): up to four DP waves where the lattice qualifies (round 5, the default) and the
    single-wave kernel for every lattice (GLOWTTS_MAS_WAVES=0; also what every other lattice takes)."""
    before = G.hip.get_knob("GLOWTTS_MAS_WAVES")
    G.hip.set_knob("GLOWTTS_MAS_WAVES", request.param)
    yield request.param
    G.hip.set_knob("GLOWTTS_MAS_WAVES", before)


def test_mas_golden_bit_exact(G, mas_kernel):
    g = load_golden("mas_cases")
    for i in range(int(g["n"])):
        v, tx, ty, want = g[f"value{i}"], g[f"tx{i}"], g[f"ty{i}"], g[f"path{i}"]
        got = G.ops.mas_path(dev(v), dev(tx), dev(ty)).cpu().numpy()
        assert got.dtype == np.float32
        assert (got == want.astype(np.float32)).all(), f"MAS golden case {i} (shape {v.shape}) differs"


def test_mas_reference_wrapper_semantics(G):
    """maximum_path(value, mask): lengths come from the mask, result has value's dtype/device (__init__.py:6-21)."""
    g = load_golden("mas_cases")
    i = 4
    v, tx, ty, want = g[f"value{i}"], g[f"tx{i}"], g[f"ty{i}"], g[f"path{i}"]
    b, mx, my = v.shape
    mask = np.zeros_like(v)
    for j in range(b):
        mask[j, : tx[j], : ty[j]] = 1
    out = G.mas.maximum_path(dev(v), dev(mask))
    assert out.is_cuda and out.dtype == torch.float32
    assert (out.cpu().numpy() == want).all()


@pytest.mark.parametrize("b,tx,ty", [(32, 160, 800), (8, 100, 400), (5, 257, 1000), (3, 500, 520), (64, 200, 1000),
                                     # beyond the former limits: > 512 tokens; bit lattice > LDS (500 x 4000:
                                     # back-pointers go through the output buffer); odd frame count on that path
                                     (2, 700, 1500), (1, 1100, 1203), (2, 500, 4000), (1, 2048, 2100)])
def test_mas_vs_oracle_full_size(G, mas_kernel, b, tx, ty):
    from oracle import glow_oracle as O

    rng = np.random.RandomState(b * 1000 + tx)
    v = (rng.randn(b, tx, ty) * 3).astype(np.float32)
    txs = rng.randint(max(1, tx // 3), tx + 1, size=b).astype(np.int32)
    tys = np.maximum(txs, rng.randint(ty // 2, ty + 1, size=b)).astype(np.int32)
    txs[0], tys[0] = tx, ty
    got = G.ops.mas_path(dev(v), dev(txs), dev(tys)).cpu().numpy()
    mask = np.zeros_like(v)
    for j in range(b):
        mask[j, : txs[j], : tys[j]] = 1
    want = O.mas_numpy(v * mask, txs, tys)
    assert (got == want.astype(np.float32)).all()
    # structure: one token per frame, monotone, surjective
    for j in range(b):
        p = got[j, : txs[j], : tys[j]]
        assert got[j].sum() == tys[j] and (p.sum(0) == 1).all()
        idx = p.argmax(0)
        d = np.diff(idx)
        assert ((d == 0) | (d == 1)).all() and idx[0] == 0 and idx[-1] == txs[j] - 1


def test_mas_ties_and_quantised(G, mas_kernel):
    from oracle import glow_oracle as O

    rng = np.random.RandomState(5)
    v = np.round(rng.randn(6, 70, 300)).astype(np.float32)       # integers: ties everywhere
    txs = np.array([70, 64, 65, 1, 33, 2], np.int32)
    tys = np.array([300, 64, 299, 300, 34, 2], np.int32)
    got = G.ops.mas_path(dev(v), dev(txs), dev(tys)).cpu().numpy()
    mask = np.zeros_like(v)
    for j in range(6):
        mask[j, : txs[j], : tys[j]] = 1
    assert (got == O.mas_numpy(v * mask, txs, tys)).all()


@pytest.mark.parametrize("b,tx,ty", [(32, 160, 800), (6, 240, 1200), (4, 64, 64), (3, 65, 132), (5, 129, 400), (2, 256, 512),
                                     (2, 257, 640), (3, 512, 1000), (7, 1, 8), (3, 100, 20), (2, 513, 1024), (2, 100, 402)])
def test_mas_spans_and_split_launches_vs_oracle(G, mas_kernel, b, tx, ty):
    """glowtts_mas_path_spans in all its forms: search + path in one call; the search alone (path = NULL) with the path expanded
    from the span table by glowtts_mas_path_from_spans (the form the training step uses, on a side stream); first / tok against the
    oracle's path.  Lattices at the wave boundaries (64 / 65, 128 / 129, 256 / 257 rows), at the edge of what the multi-wave
    kernel takes (512 / 513 tokens, Ty % 4 != 0), ragged lengths, t_x = 1, utterances shorter than a 16-frame slab."""
    from oracle import glow_oracle as O

    rng = np.random.RandomState(b * 77 + tx + ty)
    v = (rng.randn(b, tx, ty) * 2).astype(np.float32)
    txs = rng.randint(1, tx + 1, size=b).astype(np.int32)
    tys = np.maximum(txs, rng.randint(max(1, ty // 3), ty + 1, size=b)).astype(np.int32)
    tys = np.minimum(tys, ty)
    txs = np.minimum(txs, tys)
    txs[0], tys[0] = min(tx, ty), ty
    mask = np.zeros_like(v)
    for j in range(b):
        mask[j, : txs[j], : tys[j]] = 1
    want = O.mas_numpy(v * mask, txs, tys).astype(np.float32)
    vd, txd, tyd = dev(v), dev(txs), dev(tys)
    path, first, tok = G.ops.mas_path_spans(vd, txd, tyd)
    torch.cuda.synchronize()
    assert (path.cpu().numpy() == want).all()
    first, tok = first.cpu().numpy(), tok.cpu().numpy()
    for j in range(b):
        assert (np.diff(first[j]) == want[j].sum(1)).all() and first[j, 0] == 0 and (first[j, txs[j]:] == tys[j]).all()
        assert (tok[j, : tys[j]] == want[j, :, : tys[j]].argmax(0)).all() and (tok[j, tys[j]:] == -1).all()
    supported = bool(G.hip.load().glowtts_mas_spans_supported(tx, ty))
    assert supported == (mas_kernel == 1 and ty % 4 == 0 and tx <= 512)
    if supported:                                  # the search alone, then the path from the spans on another stream
        first2 = torch.full((b, tx + 1), -7, device="cuda", dtype=torch.int32)
        tok2 = torch.full((b, ty), -7, device="cuda", dtype=torch.int32)
        path2 = torch.full((b, tx, ty), float("nan"), device="cuda")
        G.hip.call("glowtts_mas_path_spans", G.hip.ptr(vd), None, G.hip.ptr(first2), G.hip.ptr(tok2), G.hip.ptr(txd.int()),
                   G.hip.ptr(tyd.int()), b, tx, ty)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        G.hip.call_on(side.cuda_stream, "glowtts_mas_path_from_spans", G.hip.ptr(first2), G.hip.ptr(path2), b, tx, ty)
        torch.cuda.synchronize()
        assert (first2.cpu().numpy() == first).all() and (tok2.cpu().numpy() == tok).all()
        assert (path2.cpu().numpy() == want).all()
    else:
        with pytest.raises(RuntimeError, match="path may be NULL only"):
            G.hip.call("glowtts_mas_path_spans", G.hip.ptr(vd), None, G.hip.ptr(torch.empty(b, tx + 1, device="cuda", dtype=torch.int32)),
                       None, G.hip.ptr(txd.int()), G.hip.ptr(tyd.int()), b, tx, ty)



@pytest.mark.parametrize("b,c,tx,ty,mean_only", [(3, 80, 37, 101, False), (2, 80, 160, 800, True), (1, 6, 5, 9, False),
                                                   (2, 100, 60, 64, False), (2, 12, 3, 403, False)])     # (spans of ~130 frames)
def test_align_logp_and_expand_vs_oracle(G, b, c, tx, ty, mean_only):
    """csrc/align.hip against the oracle's restatement of models.py:362-376 / 383-393: the (token, frame) log-likelihood
    lattice as one contraction, the spans / frame -> token map the search kernel hands out, and z_m = attn^T x_m as a gather
    with its segment-sum backward."""
    from oracle import glow_oracle as O

    torch.manual_seed(b * 100 + tx)
    x_m = torch.randn(b, c, tx)
    x_logs = torch.zeros(b, c, tx) if mean_only else 0.3 * torch.randn(b, c, tx)
    z = torch.randn(b, c, ty)
    want = O.align_logp(x_m, x_logs, z)
    got = G.ops.align_logp(dev(x_m), None if mean_only else dev(x_logs), dev(z))
    assert rel_err(got, want) < 1e-5, rel_err(got, want)
    txs = torch.tensor([tx, max(1, tx - 3), max(1, tx // 2)][:b], dtype=torch.int32)
    tys = torch.maximum(txs, torch.tensor([ty, ty - 4, ty // 2][:b], dtype=torch.int32))
    path, first, tok = G.ops.mas_path_spans(got, txs.cuda(), tys.cuda())
    assert torch.equal(path, G.ops.mas_path(got, txs.cuda(), tys.cuda()))
    path, first, tok = path.cpu(), first.cpu(), tok.cpu()
    assert torch.equal((first[:, 1:] - first[:, :-1]).float(), path.sum(-1))
    for j in range(b):
        ty_j, tx_j = int(tys[j]), int(txs[j])
        assert torch.equal(tok[j, :ty_j].long(), path[j, :, :ty_j].argmax(0)) and (tok[j, ty_j:] == -1).all()
        assert int(first[j, 0]) == 0 and (first[j, tx_j:] == ty_j).all()
    stats = x_m.clone().requires_grad_(True)
    ref = torch.matmul(path.transpose(1, 2), stats.transpose(1, 2)).transpose(1, 2)
    r = torch.randn(b, c, ty)
    (ref * r).sum().backward()
    sd = dev(x_m).requires_grad_(True)
    out = G.ops.AlignExpandFn.apply(sd, tok.cuda(), first.cuda())
    (out * r.cuda()).sum().backward()
    assert_close(out, ref, what="expand", rtol=0, atol=0)
    assert_close(sd.grad, stats.grad, what="expand grad", rtol=1e-5, atol=1e-5)


# =============================================================================================== flows vs golden
@pytest.mark.parametrize("name", ["actnorm_c8", "actnorm_c160"])
def test_actnorm_golden(G, name):
    g = load_golden(name)
    f = load_sd(G.layers.ActNorm(g["x"].shape[1]), g)
    x = dev(g["x"]).requires_grad_(True)
    mask = dev(g["mask"])
    z, logdet = f(x, mask)
    assert_close(z, g["z"], what="z", **TIGHT)
    assert_close(logdet, g["logdet"], what="logdet", **TIGHT)
    ((z * dev(g["r"])).sum() + (logdet * dev(g["s"])).sum()).backward()
    assert_close(x.grad, g["dx"], what="dx", **TIGHT)
    check_param_grads(f, g, name)
    xr, ld = f(z.detach(), mask, reverse=True)
    assert ld is None
    assert_close(xr, g["x_rev"], what="x_rev", **TIGHT)


def test_actnorm_ddi_golden(G):
    g = load_golden("actnorm_ddi")
    f = G.layers.ActNorm(8, ddi=True).cuda()
    z, logdet = f(dev(g["x"]), dev(g["mask"]))
    assert f.initialized
    assert_close(f.logs, g["sd.logs"], what="logs", **TIGHT)
    assert_close(f.bias, g["sd.bias"], what="bias", **TIGHT)
    assert_close(z, g["z"], what="z", **TIGHT)
    assert_close(logdet, g["logdet"], what="logdet", **TIGHT)


@pytest.mark.parametrize("name,n_split", [("invconv_c8_s4", 4), ("invconv_c8_s2", 2), ("invconv_c160_s4", 4)])
def test_invconv_golden(G, name, n_split):
    g = load_golden(name)
    f = load_sd(G.layers.InvConvNear(g["x"].shape[1], n_split=n_split), g)
    x = dev(g["x"]).requires_grad_(True)
    mask = dev(g["mask"])
    z, logdet = f(x, mask)
    assert_close(z, g["z"], what="z", **TIGHT)
    assert_close(logdet, g["logdet"], what="logdet", **TIGHT)
    ((z * dev(g["r"])).sum() + (logdet * dev(g["s"])).sum()).backward()
    assert_close(x.grad, g["dx"], what="dx", **TIGHT)
    check_param_grads(f, g, name)
    f.store_inverse()
    xr, ld = f(z.detach(), mask, reverse=True)
    assert ld is None
    assert_close(xr, g["x_rev"], what="x_rev", **TIGHT)


@pytest.mark.parametrize("b,c,t,n_split", [(3, 8, 37, 4), (2, 8, 64, 2), (4, 160, 100, 4), (32, 160, 400, 4)])
def test_actnorm_invconv_fused_vs_separate_and_oracle(G, b, c, t, n_split):
    """FlowSpecDecoder runs flows 3i, 3i+1 as ONE kernel each way (ops.ActNormInvConvFn); it must equal the two
    separate flows (golden-pinned above) and the oracle's composition (reference layers.py:196-197, 247-272).
    The fused kernels alone, through the C ABI against fp64 at their dispatch edges: tests/test_flow_kernels.py."""
    from oracle import glow_oracle as O

    torch.manual_seed(b * 1000 + c + t)
    x = torch.randn(b, c, t)
    lens = torch.randint(t // 2, t + 1, (b,))
    lens[0] = t
    mask = (torch.arange(t)[None] < lens[:, None]).float()[:, None]
    logs, bias = 0.3 * torch.randn(1, c, 1), 0.5 * torch.randn(1, c, 1)
    w = torch.linalg.qr(torch.randn(n_split, n_split))[0] + 0.1 * torch.randn(n_split, n_split)
    if torch.det(w) < 0:
        w[:, 0] = -w[:, 0]
    r, s = torch.randn(b, c, t), torch.randn(b)

    def run(fused):
        xs = x.cuda().requires_grad_(True)
        p = [v.cuda().requires_grad_(True) for v in (logs, bias, w)]
        m = mask.cuda()
        m2 = G.ops.mask2d(m)
        x_len = G.ops.mask_len(m2)
        if fused:
            z, ld = G.ops.ActNormInvConvFn.apply(xs, m2, p[0], p[1], p[2], x_len, n_split)
        else:
            y, ld1 = G.ops.ActNormFn.apply(xs, m2, p[0], p[1], x_len)
            z, ld2 = G.ops.InvConvFn.apply(y, m2, p[2], x_len, n_split)
            ld = ld1 + ld2
        ((z * r.cuda()).sum() + (ld * s.cuda()).sum()).backward()
        return [z, ld, xs.grad] + [q.grad for q in p]

    names = ["z", "logdet", "dx", "dlogs", "dbias", "dw"]
    fused, sep = run(True), run(False)
    for n, a, bb in zip(names, fused, sep):
        scale = float(bb.abs().max()) + 1e-6
        assert_close(a, bb, what=f"fused vs separate {n}", rtol=1e-4, atol=2e-5 * max(1.0, scale))

    xo = x.clone().requires_grad_(True)
    po = [v.clone().requires_grad_(True) for v in (logs, bias, w)]
    y, ld1 = O.actnorm(xo, mask, po[0], po[1])
    z, ld2 = O.invconv(y, mask, po[2], n_split)
    ((z * r).sum() + ((ld1 + ld2) * s).sum()).backward()
    want = [z, ld1 + ld2, xo.grad] + [q.grad for q in po]
    for n, a, bb in zip(names, fused, want):
        scale = float(bb.abs().max()) + 1e-6
        assert_close(a, bb, what=f"fused vs oracle {n}", rtol=2e-4, atol=5e-5 * max(1.0, scale))


@pytest.mark.parametrize("b,c,t,n_split", [(3, 12, 37, 6), (2, 160, 100, 10), (2, 160, 64, 16), (2, 80, 52, 20), (1, 64, 33, 32)])
def test_invconv_any_even_n_split_vs_oracle(G, b, c, t, n_split):
    """The reference allows every even n_split that divides the channels (layers.py:227,240); group sizes other than 2 / 4 / 8
    run on the run-time-N kernels: forward, reverse with the stored inverse, and autograd's gradients against the oracle
    (layers.py:247-272), through the module the decoder builds."""
    from oracle import glow_oracle as O

    torch.manual_seed(c * 100 + n_split)
    x = torch.randn(b, c, t)
    lens = torch.randint(t // 2, t + 1, (b,))
    lens[0] = t
    mask = (torch.arange(t)[None] < lens[:, None]).float()[:, None]
    f = G.layers.InvConvNear(c, n_split=n_split).cuda()
    with torch.no_grad():
        f.weight.add_(0.1 * torch.randn(n_split, n_split, device="cuda"))
        if torch.det(f.weight) < 0:
            f.weight[:, 0] = -f.weight[:, 0]
    r, s = torch.randn(b, c, t), torch.randn(b)
    xs = x.cuda().requires_grad_(True)
    z, ld = f(xs, mask.cuda())
    ((z * r.cuda()).sum() + (ld * s.cuda()).sum()).backward()
    xo = x.clone().requires_grad_(True)
    wo = f.weight.detach().cpu().clone().requires_grad_(True)
    zo, ldo = O.invconv(xo, mask, wo, n_split)
    ((zo * r).sum() + (ldo * s).sum()).backward()
    for name, a, bb in (("z", z, zo), ("logdet", ld, ldo), ("dx", xs.grad, xo.grad), ("dw", f.weight.grad, wo.grad)):
        scale = float(bb.abs().max()) + 1e-6
        assert_close(a, bb, what=f"n_split={n_split} {name}", rtol=2e-4, atol=5e-5 * max(1.0, scale))
    f.store_inverse()
    back, _ = f(z.detach(), mask.cuda(), reverse=True)
    assert_close(back, (x * mask).cuda(), what=f"n_split={n_split} round trip", rtol=1e-3, atol=1e-4)
    # and a decoder built with such a group size steps end to end (the blocks then run flow by flow, not as fused block nodes)
    if c == 160 and n_split == 10:
        dec = G.models.FlowSpecDecoder(80, 32, 5, 1, 2, 2, p_dropout=0.0, n_split=10, n_sqz=2).cuda().train()
        y = torch.randn(2, 80, 48, device="cuda", requires_grad=True)
        ym = torch.ones(2, 1, 48, device="cuda")
        zz, ldet = dec(y, ym)
        (zz.square().mean() + ldet.mean()).backward()
        assert torch.isfinite(zz).all() and torch.isfinite(y.grad).all()
        dec.store_inverse()
        with torch.no_grad():
            yy, _ = dec(zz.detach(), ym, reverse=True)
        assert_close(yy, y.detach(), what="decoder round trip with n_split=10", rtol=1e-3, atol=1e-3)


def test_invconv_prepare_matches_torch(G):
    torch.manual_seed(3)
    for n in (2, 4, 6, 8, 10, 16, 32):
        w = torch.randn(n, n)
        if torch.det(w) < 0:
            w[:, 0] = -w[:, 0]
        w_inv, ld = G.ops.invconv_prepare(w.cuda())
        assert_close(w_inv, torch.inverse(w.double()), what=f"inverse n={n}", rtol=1e-4, atol=1e-5)
        assert_close(ld[0], torch.logdet(w.double()), what=f"logdet n={n}", rtol=1e-5, atol=1e-5)
    w = torch.eye(4)
    w[0, 0] = -1.0                                                     # det < 0 -> NaN, as torch.logdet
    assert torch.isnan(G.ops.invconv_prepare(w.cuda())[1]).all()


@pytest.mark.usefixtures("conv_mode")
@pytest.mark.parametrize("name,sig,gin,k,dil,nl", [
    ("coupling_c8_h16_sig0_gin0", False, 0, 5, 1, 3),
    ("coupling_c8_h16_sig0_gin8", False, 8, 5, 1, 3),
    ("coupling_c8_h16_sig1_gin0", True, 0, 5, 1, 3),
    ("coupling_c8_h16_sig1_gin8", True, 8, 5, 1, 3),
    ("coupling_c8_h16_k3_d2", False, 0, 3, 2, 3),
])
def test_coupling_golden(G, name, sig, gin, k, dil, nl):
    g = load_golden(name)
    f = load_sd(G.attentions.CouplingBlock(8, 16, kernel_size=k, dilation_rate=dil, n_layers=nl, gin_channels=gin,
                                           p_dropout=0.0, sigmoid_scale=sig), g)
    x = dev(g["x"]).requires_grad_(True)
    mask = dev(g["mask"])
    gc = dev(g["g"]).requires_grad_(True) if gin else None
    z, logdet = f(x, mask, g=gc)
    assert_close(z, g["z"], what="z", **TIGHT)
    assert_close(logdet, g["logdet"], what="logdet", **TIGHT)
    ((z * dev(g["r"])).sum() + (logdet * dev(g["s"])).sum()).backward()
    assert_close(x.grad, g["dx"], what="dx", rtol=2e-4, atol=5e-5)
    if gin:
        assert_close(gc.grad, g["dg"], what="dg", rtol=2e-4, atol=5e-5)
    check_param_grads(f, g, name)
    with torch.no_grad():
        f.store_inverse()
        xr, ld = f(z.detach(), mask, g=None if gc is None else gc.detach(), reverse=True)
    assert ld is None
    assert_close(xr, g["x_rev"], what="x_rev", rtol=2e-4, atol=5e-5)


@pytest.mark.usefixtures("conv_mode")
@pytest.mark.parametrize("gin", [0, 8])
def test_wn_golden(G, gin):
    g = load_golden(f"wn_h16_gin{gin}")
    f = load_sd(G.layers.WN(16, 16, 5, 1, 3, gin_channels=gin, p_dropout=0.0), g)
    x = dev(g["x"]).requires_grad_(True)
    gc = dev(g["g"]).requires_grad_(True) if gin else None
    out = f(x, dev(g["mask"]), gc)
    assert_close(out, g["out"], what="out", **TIGHT)
    (out * dev(g["r"])).sum().backward()
    assert_close(x.grad, g["dx"], what="dx", rtol=2e-4, atol=5e-5)
    if gin:
        assert_close(gc.grad, g["dg"], what="dg", rtol=2e-4, atol=5e-5)
    check_param_grads(f, g, "wn")


def test_gate_and_squeeze_golden(G):
    g = load_golden("gate_h16")
    a, b = dev(g["a"]).requires_grad_(True), dev(g["b"]).requires_grad_(True)
    acts = G.utils.fused_add_tanh_sigmoid_multiply(a, b, torch.IntTensor([16]))
    assert_close(acts, g["acts"], what="acts", **TIGHT)
    (acts * dev(g["r"])).sum().backward()
    assert_close(a.grad, g["da"], what="da", **TIGHT)
    assert_close(b.grad, g["db"], what="db", **TIGHT)

    g = load_golden("squeeze_c6_t11")
    x = dev(g["x"]).requires_grad_(True)
    xs, ms = G.utils.squeeze(x, dev(g["mask"]), 2)
    assert_close(xs, g["x_sqz"], what="x_sqz", rtol=0, atol=0)
    assert_close(ms, g["mask_sqz"], what="mask_sqz", rtol=0, atol=0)
    xu, mu = G.utils.unsqueeze(xs, ms, 2)
    assert_close(xu, g["x_unsqz"], what="x_unsqz", rtol=0, atol=0)
    assert_close(mu, g["mask_unsqz"], what="mask_unsqz", rtol=0, atol=0)
    # backward of squeeze/unsqueeze against torch autograd of the oracle's layout shuffle
    from oracle import glow_oracle as O

    r = torch.randn_like(xu)
    (xu * r).sum().backward()
    xo = T(g["x"]).requires_grad_(True)
    xso, mso = O.squeeze(xo, T(g["mask"]), 2)
    xuo, _ = O.unsqueeze(xso, mso, 2)
    (xuo * r.cpu()).sum().backward()
    assert_close(x.grad, xo.grad, what="d squeeze/unsqueeze", rtol=0, atol=0)


MHA_CASES = ["mha_t12_w4", "mha_t4_w4", "mha_t5_w4", "mha_t12_w4_blk3", "mha_t12_nowin", "mha_t70_w4",     # d_k = 8: torch path
             "mha_c32_t70_w4", "mha_c32_t12_w4_blk3", "mha_c32_t5_w4", "mha_c32_t40_nowin", "mha_c192_t160_w4",     # MFMA kernel
             "mha_c192_t240_w4", "mha_c64_t256_w4", "mha_c192_t300_w4", "mha_c64_t512_w4"]      # ... at config 5's text length and at the kernel's size limit


@pytest.mark.parametrize("name", MHA_CASES)
def test_attention_golden(G, name):
    g = load_golden(name)
    win, blk = int(g["window"]), int(g["block"])
    ch = g["x"].shape[1]
    f = load_sd(G.attentions.MultiHeadAttention(ch, ch, 2, window_size=None if win < 0 else win, p_dropout=0.0,
                                                block_length=None if blk < 0 else blk), g)
    x = dev(g["x"]).requires_grad_(True)
    mask = dev(g["mask"])
    pair = mask.unsqueeze(2) * mask.unsqueeze(-1)
    assert f._kernel_applicable(x, x, pair) == (ch >= 32), "wrong path for this fixture"
    y = f(x, x, pair)
    assert_close(y, g["y"], what="y", **TIGHT)
    if f.attn is not None:
        assert_close(f.attn, g["p_attn"], what="p_attn", **TIGHT)
    (y * dev(g["r"])).sum().backward()
    assert_close(x.grad, g["dx"], what="dx", rtol=2e-4, atol=5e-5)
    check_param_grads(f, g, name)


def test_losses_golden(G):
    g = load_golden("losses")
    z, m, logs = (dev(g[k]).requires_grad_(True) for k in ("z", "m", "logs"))
    logdet = dev(g["logdet"]).requires_grad_(True)
    loss = G.utils.mle_loss(z, m, logs, logdet, dev(g["mask"]))
    assert_close(loss, g["loss"], what="mle", **TIGHT)
    loss.backward()
    for t, k in ((z, "dz"), (m, "dm"), (logs, "dlogs"), (logdet, "dlogdet")):
        assert_close(t.grad, g[k], what=k, **TIGHT)
    logw = dev(g["logw"]).requires_grad_(True)
    dl = G.utils.duration_loss(logw, dev(g["logw_"]), dev(g["lengths"]))
    assert_close(dl, g["dur_loss"], what="dur", **TIGHT)


# =============================================================================================== end to end vs golden
def _small_generator(G, tag):
    kw = dict(n_vocab=148, hidden_channels=32, filter_channels=64, filter_channels_dp=32, out_channels=80,
              kernel_size=3, n_heads=2, n_layers_enc=2, p_dropout=0.0, n_blocks_dec=2, kernel_size_dec=5,
              dilation_rate=1, n_block_layers=2, p_dropout_dec=0.0, n_speakers=0, gin_channels=0, n_split=4, n_sqz=2,
              sigmoid_scale=False, window_size=4, block_length=None, mean_only=True, hidden_channels_enc=32,
              hidden_channels_dec=32, prenet=True)
    if tag == "spk":
        kw.update(gin_channels=8, n_speakers=3, mean_only=False, sigmoid_scale=True)
    m = G.models.FlowGenerator(**kw)
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    return m


@pytest.mark.usefixtures("conv_mode")
@pytest.mark.parametrize("tag", ["base", "spk"])
def test_e2e_train_golden(G, tag):
    g = load_golden(f"e2e_{tag}_train")
    model = load_sd(_small_generator(G, tag), g).train()
    spk = dev(g["speaker_ids"]) if "speaker_ids" in g else None
    x, xl, y, yl = dev(g["x"]), dev(g["x_lengths"]), dev(g["y"]), dev(g["y_lengths"])
    opt = G.optimize.Adam(model.parameters(), scheduler="noam", dim_model=32, warmup_steps=4000, lr=1.0,
                          betas=(0.9, 0.98), eps=1e-9)
    opt.zero_grad()
    (z, z_m, z_logs, logdet, z_mask), (x_m, x_logs, x_mask), (attn, logw, logw_) = model(x, xl, y, yl, g=spk)
    outs = dict(z=z, z_m=z_m, z_logs=z_logs, logdet=logdet, z_mask=z_mask, x_m=x_m, x_logs=x_logs, x_mask=x_mask,
                logw=logw, logw_=logw_)
    for name, t in outs.items():
        assert rel_err(t, g[name]) < REL, f"{name}: rel err {rel_err(t, g[name]):.3e}"
        assert_close(t, g[name], what=name, rtol=5e-4, atol=1e-4)
    assert (attn.cpu().numpy().astype(np.int8) == g["attn"]).all(), "alignment differs from the reference"
    l_mle = G.utils.mle_loss(z, z_m, z_logs, logdet, z_mask)
    l_len = G.utils.duration_loss(logw, logw_, xl)
    assert_close(l_mle, g["l_mle"], what="l_mle", **TIGHT)
    assert_close(l_len, g["l_length"], what="l_length", **TIGHT)
    (l_mle + l_len).backward()
    gg = split_prefix(g, "grad.")
    named = dict(model.named_parameters())
    for k, want in gg.items():
        assert named[k].grad is not None, k
        assert_close(named[k].grad, want, what="grad " + k, rtol=2e-3, atol=2e-4)
    tn = G.utils.clip_grad_value_(model.parameters(), 5.0)
    assert abs(float(tn) - float(g["total_norm"])) <= 1e-3 * float(g["total_norm"])
    lrs = [opt.cur_lr]
    # the golden run applies the SAME (clamped) gradients three times: optimizer.step() does not touch .grad
    for _ in range(3):
        opt.step()
        lrs.append(opt.cur_lr)
    np.testing.assert_allclose(lrs, g["lrs"], rtol=1e-12)
    after = split_prefix(g, "sd_after3.")
    sd_now = model.state_dict()
    for k, want in after.items():
        assert_close(sd_now[k], want, what="after3 " + k, rtol=2e-3, atol=2e-5)
    st = opt._optim.dev_state.cpu()
    assert st[0] == 4.0 and st[1] == 4.0 and abs(float(st[2]) - g["lrs"][3]) <= 1e-6 * g["lrs"][3]


@pytest.mark.usefixtures("conv_mode")
def test_e2e_train_golden_with_recorded_dropout(G):
    """The training step WITH dropout against the REFERENCE: tests/golden/e2e_dropout_train.npz is the reference's own run
    with its F.dropout decisions recorded (pre-net 0.5, encoder 0.1 at four sites per layer, duration predictor 0.1, WN 0.05);
    the package is made to use the same decisions (ops.keep_mask_inject) and must reproduce all 11 outputs, both losses and
    every parameter gradient — every dropout path of the step (LayerNorm `_act` kernels, attention keep bytes, the encoder
    layer executor's four masks, the gated conv epilogue and conv_gate_bwd) at the fixtures' tolerances."""
    from helpers import MaskInject

    g = load_golden("e2e_dropout_train")
    kw = dict(n_vocab=148, hidden_channels=32, filter_channels=64, filter_channels_dp=32, out_channels=80,
              kernel_size=3, n_heads=2, n_layers_enc=2, p_dropout=0.1, n_blocks_dec=2, kernel_size_dec=5,
              dilation_rate=1, n_block_layers=2, p_dropout_dec=0.05, n_speakers=0, gin_channels=0, n_split=4, n_sqz=2,
              sigmoid_scale=False, window_size=4, block_length=None, mean_only=True, hidden_channels_enc=32,
              hidden_channels_dec=32, prenet=True)
    model = load_sd(G.models.FlowGenerator(**kw), g).train()
    sites = {k[5:]: (v, float(g["p." + k[5:]])) for k, v in g.items() if k.startswith("keep.")}
    x, xl, y, yl = dev(g["x"]), dev(g["x_lengths"]), dev(g["y"]), dev(g["y_lengths"])
    opt = G.optimize.Adam(model.parameters(), scheduler="noam", dim_model=32, warmup_steps=4000, lr=1.0,
                          betas=(0.9, 0.98), eps=1e-9)              # flat gradient buffers: the executors' in-place gradient path
    opt.zero_grad()
    with MaskInject(G.ops, sites, n_blocks=2, n_block_layers=2, n_enc=2) as inj:
        (z, z_m, z_logs, logdet, z_mask), (x_m, x_logs, x_mask), (attn, logw, logw_) = model(x, xl, y, yl)
    assert inj.served == set(sites), sorted(set(sites) - inj.served)      # every dropout site of the step took its decisions
    outs = dict(z=z, z_m=z_m, z_logs=z_logs, logdet=logdet, z_mask=z_mask, x_m=x_m, x_logs=x_logs, x_mask=x_mask,
                logw=logw, logw_=logw_)
    for name, t in outs.items():
        assert rel_err(t, g[name]) < REL, f"{name}: rel err {rel_err(t, g[name]):.3e}"
        assert_close(t, g[name], what=name, rtol=5e-4, atol=1e-4)
    assert (attn.cpu().numpy().astype(np.int8) == g["attn"]).all(), "alignment differs from the reference"
    l_mle = G.utils.mle_loss(z, z_m, z_logs, logdet, z_mask)
    l_len = G.utils.duration_loss(logw, logw_, xl)
    assert_close(l_mle, g["l_mle"], what="l_mle", **TIGHT)
    assert_close(l_len, g["l_length"], what="l_length", **TIGHT)
    (l_mle + l_len).backward()
    named = dict(model.named_parameters())
    for k, want in split_prefix(g, "grad.").items():
        assert named[k].grad is not None, k
        assert_close(named[k].grad, want, what="grad " + k, rtol=2e-3, atol=2e-4)


@pytest.mark.usefixtures("conv_mode")
@pytest.mark.parametrize("tag", ["base", "spk"])
def test_e2e_generate_golden(G, tag):
    gt = load_golden(f"e2e_{tag}_train")
    g = load_golden(f"e2e_{tag}_gen")
    model = load_sd(_small_generator(G, tag), gt).eval()
    model.decoder.store_inverse()
    spk = dev(g["speaker_ids"]) if "speaker_ids" in g else None
    noise = dev(g["noise"])
    orig = torch.randn_like
    torch.randn_like = lambda t, *a, **k: noise
    try:
        with torch.no_grad():
            (y, z_m, z_logs, ld, z_mask), _, (attn, logw, logw_) = model(
                dev(g["x"]), dev(g["x_lengths"]), g=spk, gen=True, noise_scale=float(g["noise_scale"]), length_scale=1.0)
    finally:
        torch.randn_like = orig
    assert ld is None
    assert (attn.cpu().numpy().astype(np.int8) == g["attn"]).all()
    for name, t in dict(y=y, z_m=z_m, z_logs=z_logs, z_mask=z_mask, logw=logw, logw_=logw_).items():
        assert rel_err(t, g[name]) < REL, f"{name}: rel err {rel_err(t, g[name]):.3e}"


# =============================================================================================== HIP vs oracle, mid size
def _oracle_pair(G, hp, seed=11, end_std=0.05):
    from oracle import glow_oracle as O

    sd = O.init_state_dict(hp, seed=seed)
    for k in list(sd):
        if k.endswith(".end.weight"):
            sd[k] = end_std * torch.randn_like(sd[k])
    m = G.models.FlowGenerator(
        n_vocab=hp.n_vocab, hidden_channels=hp.hidden_channels, filter_channels=hp.filter_channels,
        filter_channels_dp=hp.filter_channels_dp, out_channels=hp.out_channels, kernel_size=hp.kernel_size,
        n_heads=hp.n_heads, n_layers_enc=hp.n_layers_enc, p_dropout=0.0, n_blocks_dec=hp.n_blocks_dec,
        kernel_size_dec=hp.kernel_size_dec, dilation_rate=hp.dilation_rate, n_block_layers=hp.n_block_layers,
        p_dropout_dec=0.0, n_speakers=hp.n_speakers, gin_channels=hp.gin_channels, n_split=hp.n_split, n_sqz=hp.n_sqz,
        sigmoid_scale=hp.sigmoid_scale, window_size=hp.window_size, mean_only=hp.mean_only, prenet=hp.prenet)
    m.load_state_dict(sd)
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    return sd, m.cuda().train()


@pytest.mark.usefixtures("conv_mode")
def test_decoder_vs_oracle_config1_shapes(G):
    """FlowSpecDecoder forward + backward at BASELINE config 1 decoder shapes (B=8, 80 x 400, 6 blocks, H=192)."""
    from oracle import glow_oracle as O

    hp = O.HParams(n_blocks_dec=6, n_layers_enc=1)
    sd, model = _oracle_pair(G, hp)
    torch.manual_seed(0)
    b, t = 8, 400
    yl = torch.linspace(t, t // 2, b).long()
    y = torch.randn(b, 80, t) * (torch.arange(t)[None, None] < yl[:, None, None])
    mask = (torch.arange(t)[None, None] < ((yl // 2) * 2)[:, None, None]).float()
    r = torch.randn(b, 80, t)
    s = torch.randn(b)

    yd = y.cuda().requires_grad_(True)
    z, logdet = model.decoder(yd, mask.cuda())
    ((z * r.cuda()).sum() + (logdet * s.cuda()).sum()).backward()

    sdo = {k: v.clone().requires_grad_(True) for k, v in sd.items() if k.startswith("decoder.")}
    yo = y.clone().requires_grad_(True)
    zo, ldo = O.flow_decoder(sdo, yo, mask, None, hp)
    ((zo * r).sum() + (ldo * s).sum()).backward()

    assert rel_err(z, zo) < REL and rel_err(logdet, ldo) < REL, (rel_err(z, zo), rel_err(logdet, ldo))
    assert rel_err(yd.grad, yo.grad) < REL, rel_err(yd.grad, yo.grad)
    named = dict(model.named_parameters())
    worst = max((rel_err(named[k].grad, v.grad), k) for k, v in sdo.items())
    assert worst[0] < 5e-3, worst            # parameter gradients: long fp32 reductions in different orders
    # reverse path: mel back from z (the "mel output within 1e-3" target)
    with torch.no_grad():
        model.decoder.store_inverse()
        yr, _ = model.decoder(z.detach(), mask.cuda(), reverse=True)
    assert rel_err(yr, y * mask) < REL


@pytest.mark.usefixtures("conv_mode")
def test_generator_forward_vs_oracle_full_config2(G):
    """FlowGenerator.forward + mle_loss at BASELINE configs[1] in full — B=32, T_text=160, T_mel=800, 12 flow blocks, 6
    encoder layers, ragged lengths, dropout 0 — against the CPU oracle: z, log-det and the loss within 1e-3 relative
    (north star), and the alignment search bit-exact when both sides are fed the oracle's own `logp` (SURVEY.md hard part
    4: end to end, near-ties of `logp` may legitimately flip single frames)."""
    from oracle import glow_oracle as O

    hp = O.HParams(n_vocab=148)
    assert hp.n_blocks_dec == 12 and hp.n_layers_enc == 6 and hp.hidden_channels == 192
    # end convs N(0, 0.02): with the 0.05 of the smaller tests each of the 12 couplings scales its half of the tensor by up
    # to e^2, and the last-bit differences between the CPU's and the MFMA's summation orders grow to 1.3e-3 of max |z|
    sd, model = _oracle_pair(G, hp, seed=21, end_std=0.02)
    torch.manual_seed(3)
    b, tx, ty = 32, 160, 800
    yl = torch.linspace(ty, ty // 2, b).long()
    xl = (yl // 5).clamp(min=1)
    x = torch.randint(1, 148, (b, tx)) * (torch.arange(tx)[None] < xl[:, None])
    y = torch.randn(b, 80, ty) * (torch.arange(ty)[None, None] < yl[:, None, None])
    with torch.no_grad():
        (z, z_m, z_logs, logdet, z_mask), (x_m, x_logs, x_mask), (attn, logw, logw_) = model(x.cuda(), xl.cuda(), y.cuda(), yl.cuda())
        loss = G.utils.mle_loss(z, z_m, z_logs, logdet, z_mask)
        torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
        (zo, zo_m, zo_logs, ldo, zo_mask), (xo_m, xo_logs, _), (attn_o, logw_o, _) = O.generator_forward(sd, hp, x, xl, y, yl)
        loss_o = O.mle_loss(zo, zo_m, zo_logs, ldo, zo_mask)
        errs = {"z": rel_err(z, zo), "logdet": rel_err(logdet, ldo), "x_m": rel_err(x_m, xo_m), "logw": rel_err(logw, logw_o),
                "loss": abs(float(loss) - float(loss_o)) / abs(float(loss_o))}
        assert all(v < REL for v in errs.values()), " ".join(f"{k}={v:.2e}" for k, v in errs.items())
        # the search itself: same fp32 lattice in, same path out
        logp_o = O.align_logp(xo_m, xo_logs, zo)
        yl2 = (yl // 2) * 2
        got = G.mas.maximum_path_lengths(logp_o.cuda(), xl.cuda(), yl2.cuda())
        assert torch.equal(got.cpu(), attn_o.squeeze(1)), "MAS differs from the oracle on the oracle's own logp"
        # end to end the two alignments may differ only where logp has near-ties
        same = float((attn.cpu() == attn_o).float().mean())
        frames_moved = float((attn.cpu() - attn_o).abs().sum() / 2)
        assert same > 0.9999 and frames_moved <= 0.002 * float(yl2.sum()), (same, frames_moved)


@pytest.mark.usefixtures("conv_mode")
def test_full_step_vs_oracle_small_config(G):
    """Whole training step (forward, both losses, backward, clamp, Adam/Noam) vs the oracle, multi-speaker variant."""
    from oracle import glow_oracle as O

    hp = O.HParams(n_vocab=60, hidden_channels=64, filter_channels=128, filter_channels_dp=64, n_layers_enc=2,
                   n_blocks_dec=3, n_block_layers=2, n_speakers=4, gin_channels=16, mean_only=False)
    sd, model = _oracle_pair(G, hp, seed=5)
    torch.manual_seed(1)
    b, tx, ty = 4, 30, 160
    xl = torch.tensor([30, 25, 17, 9])
    yl = torch.tensor([160, 140, 101, 48])
    x = torch.randint(1, 60, (b, tx)) * (torch.arange(tx)[None] < xl[:, None])
    y = torch.randn(b, 80, ty) * (torch.arange(ty)[None, None] < yl[:, None, None])
    spk = torch.tensor([0, 3, 1, 2])

    opt = G.optimize.Adam(model.parameters(), scheduler="noam", dim_model=64, warmup_steps=4000, lr=1.0)
    from glow_tts_train.train import train_batch

    loss = train_batch(model, opt, (x.cuda(), xl.cuda(), y.cuda(), yl.cuda(), spk.cuda()), 5.0)

    sdo = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    oopt = O.AdamNoam({k: v for k, v in sdo.items()}, dim_model=64)
    oloss, frames = O.train_step(sdo, hp, oopt, (x, xl, y, yl, spk), 5.0)
    assert frames == int(yl.sum())
    assert abs(float(loss) - oloss) <= 1e-3 * abs(oloss), (float(loss), oloss)
    # gradients (already clamped in place on both sides) agree tensor by tensor
    named = dict(model.named_parameters())
    gmax = max(float(v.grad.abs().max()) for v in sdo.values() if v.grad is not None)
    for k, v in sdo.items():
        if v.grad is None:
            continue
        # per-tensor relative check with a floor at 1e-5 of the largest gradient in the model: some gradients are
        # mathematically zero (e.g. the key-projection bias: softmax is invariant to it) and hold only rounding noise
        assert_close(named[k].grad, v.grad, what="grad " + k, rtol=0,
                     atol=5e-3 * float(v.grad.abs().max()) + 1e-5 * gmax)
    # the first Adam update is lr * g / (|g| + eps): sign-like, so it is only comparable where the gradient is
    # well above rounding noise; there the two updates must agree (the arithmetic itself is pinned bit-tight by
    # test_e2e_train_golden, which replays the reference's own three updates)
    now = model.state_dict()
    lr0 = O.noam_lr(1, 64, 4000)
    for k, v in sdo.items():
        if v.grad is None:
            continue
        g = v.grad
        big = g.abs() > 1e-3 * gmax          # relative to the model's largest gradient, not the tensor's own
        if not bool(big.any()):
            continue
        upd_o = (v.detach() - sd[k])[big]
        upd_h = (now[k].cpu() - sd[k])[big]
        assert float((upd_h - upd_o).abs().max()) <= 0.05 * lr0, k


# =============================================================================================== full-size properties
def test_full_size_decoder_roundtrip_and_mas_properties(G):
    """BASELINE config 2 sizes (B=32, T_mel=800, T_text=160, 12 blocks): size-independent checks only."""
    from oracle import glow_oracle as O

    hp = O.HParams()
    sd, model = _oracle_pair(G, hp, seed=2, end_std=0.005)      # well-conditioned couplings: |logs| stays O(0.1)
    torch.manual_seed(4)
    b, t = 32, 800
    y = torch.randn(b, 80, t, device="cuda")
    mask = torch.ones(b, 1, t, device="cuda")
    with torch.no_grad():
        z, logdet = model.decoder(y, mask)
        model.decoder.store_inverse()
        yr, _ = model.decoder(z, mask, reverse=True)
    assert torch.isfinite(z).all() and torch.isfinite(logdet).all()
    assert rel_err(yr, y) < REL
    # linearity of the log-det in the number of frames: an utterance of half the length has half the ActNorm+InvConv part
    v = torch.randn(b, 160, t, device="cuda")
    tx = torch.full((b,), 160, dtype=torch.int32, device="cuda")
    ty = torch.full((b,), t, dtype=torch.int32, device="cuda")
    p = G.ops.mas_path(v, tx, ty)
    assert (p.sum(1) == 1).all() and p.sum() == b * t
    idx = p.argmax(1)
    d = idx[:, 1:] - idx[:, :-1]
    assert ((d == 0) | (d == 1)).all() and (idx[:, 0] == 0).all() and (idx[:, -1] == 159).all()
    # idempotence: the path of a lattice that rewards exactly that path is the same path
    assert (G.ops.mas_path(p * 10.0, tx, ty) == p).all()


@pytest.mark.parametrize("name,b,t_text,t_mel,blocks,spk", [
    ("config3-shapes", 64, 200, 1000, 12, False),       # BASELINE configs[2] sizes (arithmetic here is fp32)
    ("config5", 48, 240, 1200, 20, True),               # BASELINE configs[4]: speaker-conditioned, 20 blocks, long
])
def test_full_size_other_configs_step_and_roundtrip(G, name, b, t_text, t_mel, blocks, spk):
    """The larger BASELINE configurations at full size, ragged lengths: size-independent checks — decoder -> inverse
    gives the mel back, the alignment is a monotonic path per utterance, the log-det of an utterance does not depend
    on what else is in the batch, one full optimisation step leaves finite parameters and moves them."""
    from oracle import glow_oracle as O
    from glow_tts_train.train import train_batch

    hp = O.HParams(n_blocks_dec=blocks, n_speakers=4 if spk else 0, gin_channels=64 if spk else 0)
    sd, model = _oracle_pair(G, hp, seed=3, end_std=0.005)
    gen = torch.Generator().manual_seed(6)
    yl = torch.linspace(t_mel, t_mel // 2, b).long()
    xl = (yl // 5).clamp(min=1)
    x = (torch.randint(1, 148, (b, t_text), generator=gen) * (torch.arange(t_text)[None] < xl[:, None])).cuda()
    y = (torch.randn(b, 80, t_mel, generator=gen) * (torch.arange(t_mel)[None, None] < yl[:, None, None])).cuda()
    ids = (torch.arange(b) % 4).cuda() if spk else None
    xl, yl = xl.cuda(), yl.cuda()

    with torch.no_grad():
        (z, z_m, z_logs, logdet, z_mask), _, (attn, logw, logw_) = model(x, xl, y, yl, g=ids)
        assert all(torch.isfinite(t).all() for t in (z, z_m, z_logs, logdet, logw, logw_))
        # alignment: one text position per valid frame, non-decreasing, ending on the last text position
        path = attn[:, 0]                                              # (B, T_text, T_mel)
        frames = z_mask[:, 0].sum(1).long()
        assert (path.sum(1) == z_mask[:, 0]).all()
        idx = path.argmax(1)
        for i in (0, b // 2, b - 1):
            n = int(frames[i])
            d = idx[i, 1:n] - idx[i, :n - 1]
            assert ((d == 0) | (d == 1)).all() and idx[i, 0] == 0 and idx[i, n - 1] == int(xl[i]) - 1
        # batch independence: the shortest utterance alone gives the same latent and log-det
        g1 = None if ids is None else model.emb_g(ids[-1:]).unsqueeze(-1)
        g_all = None if ids is None else model.emb_g(ids).unsqueeze(-1)
        if g1 is not None:
            g1, g_all = torch.nn.functional.normalize(g1, dim=1), torch.nn.functional.normalize(g_all, dim=1)
        n = int(frames[-1])
        z1, ld1 = model.decoder(y[-1:, :, :n].contiguous(), z_mask[-1:, :, :n].contiguous(), g=g1)
        assert rel_err(z1, z[-1:, :, :n]) < REL and rel_err(ld1, logdet[-1:]) < REL
        # invertibility at full size
        model.decoder.store_inverse()
        yr, _ = model.decoder(z, z_mask, g=g_all, reverse=True)
        assert rel_err(yr, y[:, :, :z.shape[2]] * z_mask) < REL

    opt = G.optimize.Adam(model.parameters(), scheduler="noam", dim_model=192, warmup_steps=4000, lr=1.0)
    before = opt._optim.flat_p.clone()
    loss = train_batch(model, opt, (x, xl, y, yl, ids), 5.0)
    assert torch.isfinite(loss) and torch.isfinite(opt._optim.flat_p).all() and torch.isfinite(opt._optim.flat_g).all()
    assert (opt._optim.flat_p != before).float().mean() > 0.5


# =============================================================================================== MFMA conv kernels
@pytest.mark.parametrize("b,cin,cout,t,k,dil,mask_out,slice_in", [
    (3, 80, 192, 50, 1, 1, True, True),       # coupling start conv: channel slice consumed in place, masked output
    (2, 192, 384, 400, 5, 1, False, False),   # WN in-layer shape, 80-frame tiles
    (2, 192, 160, 77, 1, 1, False, False),    # end conv, ragged T (64-frame tiles, partial rows)
    (2, 24, 36, 130, 3, 2, True, False),      # dilation 2, small odd channel counts
    (1, 5, 4, 16, 5, 3, False, False),        # halo wider than the tile interior
    (4, 192, 192, 160, 3, 1, False, False),
    (3, 80, 192, 48, 1, 1, True, True),       # pipelined path (T % 4 == 0) with slice input + masked output
    (2, 40, 72, 120, 3, 2, True, False),      # pipelined, 3 taps dilation 2, T % 40 == 0 weight-grad chunks
    (2, 192, 384, 96, 5, 2, False, False),    # pipelined 5 taps dilation 2
    (1, 16, 32, 20, 5, 4, False, False),      # halo 16 > 12: generic fallback
    (32, 80, 192, 400, 1, 1, True, True),     # config-2 start conv: 480 workgroups -> 80-frame tiles (PLAIN epilogue)
    (32, 192, 768, 160, 3, 1, False, False),  # config-2 encoder FFN conv: under-filled grid -> 32-frame tiles
])
def test_conv1d_fn_vs_torch(G, b, cin, cout, t, k, dil, mask_out, slice_in):
    from glow_tts_train import convops

    torch.manual_seed(b * 100 + cin)
    full = torch.randn(b, cin * (2 if slice_in else 1), t)
    v = torch.randn(cout, cin, k) * (cin * k) ** -0.5
    g = torch.rand(cout, 1, 1) + 0.5
    bias = torch.randn(cout) * 0.1
    lengths = torch.linspace(t, max(1, t // 2), b).long()
    mask = (torch.arange(t)[None, :] < lengths[:, None]).float()
    r = torch.randn(b, cout, t)

    def ref(use_g):
        xf = full.clone().requires_grad_(True)
        vv, gg, bb = v.clone().requires_grad_(True), g.clone().requires_grad_(True), bias.clone().requires_grad_(True)
        w = vv * (gg / vv.flatten(1).norm(dim=1).view(-1, 1, 1)) if use_g else vv
        y = torch.nn.functional.conv1d(xf[:, :cin], w, bb, dilation=dil, padding=(k * dil - dil) // 2)
        if mask_out:
            y = y * mask.unsqueeze(1)
        (y * r).sum().backward()
        return y, xf.grad, vv.grad, gg.grad if use_g else None, bb.grad

    for use_g in (True, False):
        y0, dx0, dv0, dg0, db0 = ref(use_g)
        xf = full.cuda().requires_grad_(True)
        vv, bb = v.cuda().requires_grad_(True), bias.cuda().requires_grad_(True)
        gg = g.cuda().requires_grad_(True) if use_g else None
        y = convops.Conv1dFn.apply(xf[:, :cin], vv, gg, bb, mask.cuda(), False, mask_out, dil)
        (y * r.cuda()).sum().backward()
        assert_close(y, y0, what="y", rtol=1e-4, atol=1e-4)
        assert_close(xf.grad, dx0, what="dx", rtol=1e-4, atol=1e-4)
        # weight gradients sum B*T products in fp32 (split-K atomics here, a different order in the CPU reference):
        # the absolute error scales with the largest entry of the reduction, not with each small entry
        assert_close(vv.grad, dv0, what="dv", rtol=2e-4, atol=2e-4 * max(1.0, float(dv0.abs().max())))
        assert_close(bb.grad, db0, what="db", rtol=2e-4, atol=2e-4 * max(1.0, float(db0.abs().max())))
        if use_g:
            assert_close(gg.grad, dg0, what="dg", rtol=2e-4, atol=2e-4 * max(1.0, float(dg0.abs().max())))


def test_conv_grads_accumulate_in_place_when_grad_exists(G):
    """With .grad pre-allocated (flat-buffer optimizer) the operators add into it and hand autograd None."""
    from glow_tts_train import convops

    torch.manual_seed(0)
    x = torch.randn(2, 8, 40, device="cuda")
    v = torch.randn(12, 8, 3, device="cuda", requires_grad=True)
    bias = torch.zeros(12, device="cuda", requires_grad=True)
    m = torch.ones(2, 40, device="cuda")
    convops.Conv1dFn.apply(x, v, None, bias, m, False, False, 1).sum().backward()
    gv, gb = v.grad.clone(), bias.grad.clone()
    before = v.grad.data_ptr()
    convops.Conv1dFn.apply(x, v, None, bias, m, False, False, 1).sum().backward()       # second backward: in place, 2x
    assert v.grad.data_ptr() == before
    assert_close(v.grad, 2 * gv, rtol=1e-5, atol=1e-5)
    assert_close(bias.grad, 2 * gb, rtol=1e-5, atol=1e-5)


def test_wn_dropout_path_matches_manual_mask(G):
    """Training-mode dropout inside WN (layers.py:147): the stack's own keep-masks (read back through ops.keep_mask_tap) applied
    by hand to the oracle's convolutions; forward and backward agree."""
    from oracle import glow_oracle as O

    torch.manual_seed(3)
    H, L, b, t, p = 16, 3, 2, 48, 0.3
    wn = G.layers.WN(16, H, 5, 1, L, gin_channels=0, p_dropout=p).cuda().train()
    x = torch.randn(b, H, t, device="cuda", requires_grad=True)
    mask = torch.ones(b, 1, t, device="cuda")
    mask[1, :, 30:] = 0
    r = torch.randn(b, H, t, device="cuda")
    taken = []
    G.ops.keep_mask_tap = lambda site, m, pd: taken.append(m.clone())
    try:
        out = wn(x, mask)
    finally:
        G.ops.keep_mask_tap = None
    (out * r).sum().backward()
    assert len(taken) == 1 and taken[0].shape == (L, b, 2 * H, t)        # one generator call for the stack
    keeps = list(taken[0].float())
    sd = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in wn.state_dict().items()}
    xo = x.detach().cpu().clone().requires_grad_(True)
    cur, skip = xo, 0
    for i in range(L):
        pre = O.conv1d(sd, f"in_layers.{i}", cur) * keeps[i].cpu() / (1 - p)
        acts = O.gate(pre, torch.zeros_like(pre), H)
        rs = O.conv1d(sd, f"res_skip_layers.{i}", acts)
        if i < L - 1:
            cur = (cur + rs[:, :H]) * mask.cpu()
            skip = skip + rs[:, H:]
        else:
            skip = skip + rs
    want = skip * mask.cpu()
    (want * r.cpu()).sum().backward()
    assert_close(out, want, what="out", rtol=1e-4, atol=1e-4)
    assert_close(x.grad, xo.grad, what="dx", rtol=2e-4, atol=2e-4)
    named = dict(wn.named_parameters())
    for k, vref in sd.items():
        assert_close(named[k].grad, vref.grad, what="grad " + k, rtol=5e-4, atol=5e-4)


@pytest.mark.parametrize("t,lens", [(50, (50, 31, 7)), (300, (300, 211, 64)), (640, (640, 513, 90))],
                         ids=["t50", "t300-long-form", "t640-beyond-the-strips"])
def test_attention_dropout_matches_manual_mask(G, t, lens):
    """Training-mode attention dropout (attentions.py:251): the kernel's keep-mask read back (ops.keep_mask_tap) and handed to the
    index-based torch composition (ops.keep_mask_inject) — outputs and every gradient agree."""
    torch.manual_seed(5)
    ch, b, p = 64, 3, 0.25
    f = G.attentions.MultiHeadAttention(ch, ch, 2, window_size=4, p_dropout=p).cuda().train()
    x = torch.randn(b, ch, t, device="cuda", requires_grad=True)
    lens = torch.tensor(lens, device="cuda")
    mask = (torch.arange(t, device="cuda")[None, :] < lens[:, None]).float().unsqueeze(1)
    pair = mask.unsqueeze(2) * mask.unsqueeze(-1)
    r = torch.randn(b, ch, t, device="cuda")
    taken = []
    G.ops.keep_mask_tap = lambda site, m, pd: taken.append((site, m.clone(), pd))
    try:
        y = f(x, x, pair)
    finally:
        G.ops.keep_mask_tap = None
    assert len(taken) == 1 and taken[0][1].shape == (b, 2, t, t) and taken[0][2] == p
    (y * r).sum().backward()
    got = [x.grad.clone()] + [p_.grad.clone() for p_ in f.parameters()]
    x.grad = None
    f.zero_grad()
    G.ops.keep_mask_inject = lambda site, shape, pd: taken[0][1]
    try:
        q, k, v = f.conv_q(x), f.conv_k(x), f.conv_v(x)
        o, _ = f._attention_general(q, k, v, pair)
    finally:
        G.ops.keep_mask_inject = None
    y2 = f.conv_o(o)
    (y2 * r).sum().backward()
    want = [x.grad] + [p_.grad for p_ in f.parameters()]
    assert_close(y, y2, what="y", rtol=1e-4, atol=1e-4)
    for a, e in zip(got, want):
        assert_close(a, e, what="grad", rtol=5e-4, atol=5e-4)


@pytest.mark.parametrize("t,ch,win,blk", [(160, 192, 4, None), (256, 64, 7, None), (200, 32, 4, 20), (33, 256, 2, None),
                                          (240, 192, 4, None), (256, 192, 7, None),      # config 5 / the short form's limit
                                          (257, 192, 4, None), (300, 192, 7, 30), (384, 64, 4, None), (500, 32, 2, None),
                                          (512, 192, 7, None),                           # the LONG form: 256 < T <= 512
                                          (513, 32, 2, None), (600, 192, 4, None), (777, 64, 7, 50),
                                          (1024, 192, 4, None)])                         # beyond the strips: csrc/attention_long.hip
def test_attention_kernel_vs_general_path(G, t, ch, win, blk):
    torch.manual_seed(t)
    b = 2
    f = G.attentions.MultiHeadAttention(ch, ch, 2, window_size=win, p_dropout=0.0, block_length=blk).cuda().eval()
    x = torch.randn(b, ch, t, device="cuda", requires_grad=True)
    lens = torch.tensor([t, max(1, t // 3)], device="cuda")
    mask = (torch.arange(t, device="cuda")[None, :] < lens[:, None]).float().unsqueeze(1)
    pair = mask.unsqueeze(2) * mask.unsqueeze(-1)
    r = torch.randn(b, ch, t, device="cuda")
    q, k, v = f.conv_q(x), f.conv_k(x), f.conv_v(x)
    assert f._kernel_applicable(q, k, pair)
    o1, p1 = f.attention(q, k, v, pair)
    (o1 * r).sum().backward()
    g1 = [x.grad.clone(), f.emb_rel_k.grad.clone(), f.emb_rel_v.grad.clone()]
    x.grad = None
    f.zero_grad()
    q, k, v = f.conv_q(x), f.conv_k(x), f.conv_v(x)
    o2, p2 = f._attention_general(q, k, v, pair)
    (o2 * r).sum().backward()
    g2 = [x.grad, f.emb_rel_k.grad, f.emb_rel_v.grad]
    assert_close(o1, o2, what="out", rtol=1e-4, atol=1e-4)
    assert_close(p1, p2, what="p_attn", rtol=1e-4, atol=1e-5)
    for a, e, n in zip(g1, g2, ("dx", "demb_k", "demb_v")):
        assert_close(a, e, what=n, rtol=5e-4, atol=5e-4)


@pytest.mark.parametrize("bf16_mma", [False, True])
@pytest.mark.parametrize("t", [128, 160, 192, 96, 320])
def test_attention_backward_is_bit_identical_from_run_to_run(G, t, bf16_mma):
    """dS, dQ, dK, dV have no atomics in them: thirty launches on the same inputs must agree bit for bit.  Round 4: they did
    not — at T = 128 / 160 / 192 the score gradient of the LAST 16-key tile came out with register [3] of its accumulators one
    k step short in ~25 % of launches (rows 3, 7, 11, 15 of the last two row tiles; 0.07 on a tensor of 0.33): the compiler had
    left no wait between the tile's last MFMA and the accumulator read behind a taken forward branch (csrc/common.hpp:
    mfma_settle; tools/mfma_hazard_scan.py checks the built library for that pattern)."""
    from glow_tts_train._hip import call

    ptr = lambda x: None if x is None else x.data_ptr()                    # noqa: E731
    torch.manual_seed(t)
    b, h, dk, w = 3, 2, 96, 4
    q, k, v, dout = (torch.randn(b, h * dk, t, device="cuda") for _ in range(4))
    lens = torch.tensor([t, (3 * t) // 4, t // 2 - 3], device="cuda")
    m2 = (torch.arange(t, device="cuda")[None] < lens[:, None]).float().contiguous()
    ek, ev = (torch.randn(1, 2 * w + 1, dk, device="cuda") * dk ** -0.5 for _ in range(2))
    p = torch.empty(b, h, t, t, device="cuda")
    out = torch.empty_like(q)
    call("glowtts_rel_attn_fwd_ex", ptr(q), ptr(k), ptr(v), ptr(ek), ptr(ev), ptr(m2), None, 1.0, ptr(p), ptr(out), b, h, t, dk, w, 1,
         -1, int(bf16_mma))
    for it in range(20):                                   # the forward kernels had the same early-read paths (same template)
        p2 = torch.full_like(p, float("nan"))
        out2 = torch.full_like(out, float("nan"))
        call("glowtts_rel_attn_fwd_ex", ptr(q), ptr(k), ptr(v), ptr(ek), ptr(ev), ptr(m2), None, 1.0, ptr(p2), ptr(out2), b, h, t, dk, w,
             1, -1, int(bf16_mma))
        torch.cuda.synchronize()
        assert torch.equal(p2, p) and torch.equal(out2, out), (it, float((out2 - out).abs().max()))
    first = None
    for it in range(30):
        ds = torch.full((b, h, t, t), float("nan"), device="cuda")
        dq, dkk, dv = (torch.full_like(q, float("nan")) for _ in range(3))
        dek, dev_ = torch.zeros_like(ek), torch.zeros_like(ev)
        call("glowtts_rel_attn_bwd_ex", ptr(dout), ptr(q), ptr(k), ptr(v), ptr(ek), ptr(ev), ptr(m2), None, 1.0, ptr(p), ptr(ds),
             ptr(dq), ptr(dkk), ptr(dv), ptr(dek), ptr(dev_), b, h, t, dk, w, 1, -1, int(bf16_mma))
        torch.cuda.synchronize()
        got = (ds, dq, dkk, dv)
        if first is None:
            first = got
            assert all(bool(torch.isfinite(x).all()) for x in got)
            continue
        for name, a, e in zip(("ds", "dq", "dk", "dv"), got, first):
            assert torch.equal(a, e), (it, name, float((a - e).abs().max()))


@pytest.mark.parametrize("b,c,t,with_res", [(3, 192, 160, True), (2, 32, 37, False), (1, 5, 70, True), (2, 1024, 24, True)])
def test_chan_layernorm_vs_torch(G, b, c, t, with_res):
    # (1 024 channels: wider than the register-resident kernels take — the module then composes framework operators on the
    #  device instead of refusing to build; same results)
    from oracle import glow_oracle as O

    torch.manual_seed(c)
    ln = G.layers.LayerNorm(c).cuda()
    with torch.no_grad():
        ln.gamma.copy_(torch.rand(c) + 0.5)
        ln.beta.copy_(torch.randn(c) * 0.1)
    x = (torch.randn(b, c, t) * 2 + 0.3).cuda().requires_grad_(True)
    res = torch.randn(b, c, t).cuda().requires_grad_(True) if with_res else None
    r = torch.randn(b, c, t).cuda()
    y = ln(x, res=res)
    (y * r).sum().backward()
    xo = x.detach().cpu().requires_grad_(True)
    ro = res.detach().cpu().requires_grad_(True) if with_res else None
    go, bo = ln.gamma.detach().cpu().requires_grad_(True), ln.beta.detach().cpu().requires_grad_(True)
    yo = O.channel_layer_norm(xo + ro if with_res else xo, go, bo)
    (yo * r.cpu()).sum().backward()
    assert_close(y, yo, what="y", rtol=1e-4, atol=1e-5)
    assert_close(x.grad, xo.grad, what="dx", rtol=1e-4, atol=2e-5)
    if with_res:
        assert_close(res.grad, ro.grad, what="dres", rtol=1e-4, atol=2e-5)
    assert_close(ln.gamma.grad, go.grad, what="dgamma", rtol=2e-4, atol=2e-4)
    assert_close(ln.beta.grad, bo.grad, what="dbeta", rtol=2e-4, atol=2e-4)


@pytest.mark.parametrize("b,c,t", [(3, 192, 160), (2, 256, 37), (1, 5, 70), (2, 800, 20)])
@pytest.mark.parametrize("relu_in,relu_out,p", [(True, False, 0.0), (False, True, 0.0), (False, True, 0.5), (True, False, 0.3)])
def test_chan_layernorm_fused_relu_dropout_vs_torch(G, b, c, t, relu_in, relu_out, p):
    """The ReLU before / the ReLU and dropout after a LayerNorm inside its kernels (pre-net: layers.py:73-80; duration
    predictor: models.py:44-50) against the torch composition with the SAME keep-mask (read back from where y is zero)."""
    from oracle import glow_oracle as O

    torch.manual_seed(c + int(10 * p))
    ln = G.layers.LayerNorm(c).cuda()
    with torch.no_grad():
        ln.gamma.copy_(torch.rand(c) + 0.5)
        ln.beta.copy_(torch.randn(c) * 0.1)
    x = (torch.randn(b, c, t) * 2 + 0.3).cuda().requires_grad_(True)
    r = torch.randn(b, c, t).cuda()
    y = ln(x, relu_in=relu_in, relu_out=relu_out, p_drop=p)
    (y * r).sum().backward()

    xo = x.detach().cpu().requires_grad_(True)
    go, bo = ln.gamma.detach().cpu().requires_grad_(True), ln.beta.detach().cpu().requires_grad_(True)
    v = O.channel_layer_norm(torch.relu(xo) if relu_in else xo, go, bo)
    if relu_out:
        v = torch.relu(v)
    keep = torch.ones_like(v)
    if p > 0:
        # an element was dropped iff y is zero where the un-dropped value is not
        keep = ((y.detach().cpu() != 0) | (v.detach() == 0)).float()
        live = v.detach() != 0                                 # (where the value itself is zero the mask cannot be read back)
        frac = float(keep[live].mean())
        assert abs(frac - (1 - p)) < 0.05 + 2.0 / float(live.sum()) ** 0.5, frac
        v = v * keep / (1 - p)
    (v * r.cpu()).sum().backward()
    assert_close(y, v, what="y", rtol=1e-4, atol=2e-5)
    assert_close(x.grad, xo.grad, what="dx", rtol=1e-4, atol=4e-5)
    assert_close(ln.gamma.grad, go.grad, what="dgamma", rtol=2e-4, atol=4e-4)
    assert_close(ln.beta.grad, bo.grad, what="dbeta", rtol=2e-4, atol=4e-4)


def test_embedding_kernels_vs_torch(G):
    """h = emb(ids) * sqrt(H) as (B, H, T) (models.py:121-122) and its backward (segment sum per vocabulary entry)."""
    from glow_tts_train import convops

    torch.manual_seed(3)
    V, H, B, T = 148, 192, 5, 67
    w = torch.randn(V, H, device="cuda", requires_grad=True)
    ids = torch.randint(0, V, (B, T), device="cuda")
    ids[:, -9:] = 0                                           # a padded tail: id 0 repeated
    r = torch.randn(B, H, T, device="cuda")
    scale = H ** 0.5
    out = convops.EmbedFn.apply(ids, w, scale)
    (out * r).sum().backward()
    w2 = w.detach().clone().requires_grad_(True)
    ref = (torch.nn.functional.embedding(ids, w2) * scale).transpose(1, 2)
    (ref * r).sum().backward()
    assert torch.equal(out, ref.contiguous())
    assert_close(w.grad, w2.grad, what="dweight", rtol=1e-5, atol=1e-4)
    # the segment sum walks a token's positions in ascending order whatever the scheduling: bit-identical from run to run,
    # also at the benchmark's size (32 x 160 positions = three 2 048-position chunks per vocabulary entry)
    for (b_, t_) in ((B, T), (32, 160)):
        ids_ = torch.randint(0, V, (b_, t_), device="cuda")
        r_ = torch.randn(b_, H, t_, device="cuda")
        grads = []
        for _ in range(3):
            w3 = w.detach().clone().requires_grad_(True)
            (convops.EmbedFn.apply(ids_, w3, scale) * r_).sum().backward()
            grads.append(w3.grad.clone())
        assert torch.equal(grads[0], grads[1]) and torch.equal(grads[0], grads[2])
        w4 = w.detach().clone().requires_grad_(True)
        ((torch.nn.functional.embedding(ids_, w4) * scale).transpose(1, 2) * r_).sum().backward()
        assert_close(grads[0], w4.grad, what="dweight", rtol=1e-5, atol=2e-4)
    # an id outside the vocabulary (nn.Embedding: device assert) poisons its column instead of training on a clamped id
    bad = ids.clone()
    bad[1, 3], bad[2, 5] = V, -1
    w5 = w.detach().clone().requires_grad_(True)
    o5 = convops.EmbedFn.apply(bad, w5, scale)
    assert torch.isnan(o5[1, :, 3]).all() and torch.isnan(o5[2, :, 5]).all()
    ok = torch.ones(B, T, dtype=torch.bool, device="cuda")
    ok[1, 3] = ok[2, 5] = False
    assert torch.equal(o5.transpose(1, 2)[ok], out.detach().transpose(1, 2)[ok])
    # the model's encoder uses it: one launch, no (B, T, H) tensor
    enc = G.models.TextEncoder(V, 80, 192, 768, 256, 2, 1, 3, 0.0, window_size=4, mean_only=True, prenet=True).cuda()
    xl = torch.full((B,), T, device="cuda")
    x_m, _, logw, _ = enc(ids.clamp(min=1), xl)
    assert torch.isfinite(x_m).all() and torch.isfinite(logw).all()


def test_coupling_block_grouped_and_linked_paths_match_plain_autograd(G):
    """With pre-allocated .grad tensors (the flat-buffer optimizer's situation) a coupling block packs its start / end convs
    in one launch, un-packs their gradients in one launch (convops.ConvGroup) and shares ONE input-gradient buffer between
    the affine apply and the start conv (ops.GradLink).  Same block, same inputs, gradients left to plain autograd
    (.grad = None): every gradient must agree."""
    torch.manual_seed(21)
    blk = G.attentions.CouplingBlock(160, 192, kernel_size=5, dilation_rate=1, n_layers=4, p_dropout=0.0).cuda()
    with torch.no_grad():
        blk.end.weight.normal_(0, 0.02)
        blk.end.bias.normal_(0, 0.02)
    b, t = 4, 96
    x0 = torch.randn(b, 160, t, device="cuda")
    lens = torch.tensor([96, 80, 64, 50], device="cuda")
    mask = (torch.arange(t, device="cuda")[None] < lens[:, None]).float()[:, None]
    r, s = torch.randn(b, 160, t, device="cuda"), torch.randn(b, device="cuda")

    def run(prealloc):
        for p in blk.parameters():
            p.grad = torch.zeros_like(p) if prealloc else None
        x = (x0 * mask).clone().requires_grad_(True)
        z, ld = blk(x, mask)
        ((z * r).sum() + (ld * s).sum()).backward()
        G.hip.join_side_streams()
        from glow_tts_train import convops
        convops.flush_groups()
        torch.cuda.synchronize()
        return z.detach(), ld.detach(), x.grad.clone(), {k: p.grad.clone() for k, p in blk.named_parameters()}

    z0, l0, dx0, g0 = run(False)
    assert not blk._conv_group.active
    z1, l1, dx1, g1 = run(True)
    assert blk._conv_group.active
    assert_close(z1, z0, what="z", rtol=1e-6, atol=1e-6)
    assert_close(l1, l0, what="logdet", rtol=1e-6, atol=1e-5)
    assert_close(dx1, dx0, what="dx", rtol=1e-4, atol=1e-5 * float(dx0.abs().max()))
    for k in g0:
        assert_close(g1[k], g0[k], what=f"grad {k}", rtol=2e-4, atol=2e-5 * max(1.0, float(g0[k].abs().max())))


def test_direct_grads_switch_routes_gradients_through_autograd(G):
    """`convops.set_direct_grads(False)` (what a DistributedDataParallel wrap needs): every parameter gradient comes back
    through autograd's AccumulateGrad — hooks fire for all of them — and equals the in-place path's result."""
    from glow_tts_train import convops

    torch.manual_seed(41)
    blk = G.attentions.CouplingBlock(32, 48, kernel_size=3, dilation_rate=1, n_layers=2, p_dropout=0.0).cuda()
    with torch.no_grad():
        blk.end.weight.normal_(0, 0.05)
    x0 = torch.randn(2, 32, 40, device="cuda")
    mask = torch.ones(2, 1, 40, device="cuda")
    r = torch.randn(2, 32, 40, device="cuda")
    fired = set()
    hooks = [p.register_post_accumulate_grad_hook(lambda p_, n=n: fired.add(n)) for n, p in blk.named_parameters()]
    res = {}
    try:
        for direct in (True, False):
            convops.set_direct_grads(direct)
            fired.clear()
            for p in blk.parameters():
                p.grad = torch.zeros_like(p)
            x = x0.clone().requires_grad_(True)
            z, ld = blk(x, mask)
            ((z * r).sum() + ld.sum()).backward()
            convops.flush_groups()
            torch.cuda.synchronize()
            res[direct] = ({k: p.grad.clone() for k, p in blk.named_parameters()}, set(fired))
    finally:
        convops.set_direct_grads(None)               # back to the automatic choice
        for h in hooks:
            h.remove()
    names = {n for n, _ in blk.named_parameters()}
    assert res[False][1] == names, f"no AccumulateGrad event for {sorted(names - res[False][1])}"
    for k in names:
        want = res[True][0][k]
        assert_close(res[False][0][k], want, what=f"grad {k}", rtol=2e-4, atol=2e-5 * max(1.0, float(want.abs().max())))


def test_wn_native_executor_matches_layer_by_layer_path(G):
    """csrc/wn_stack.hip queues a whole WN stack from C (forward by default, backward with GLOWTTS_WN_NATIVE=both); the
    same stack driven launch by launch from Python ("off") is the reference.  Dropout on, ragged mask, pre-allocated grads."""
    from glow_tts_train import convops

    torch.manual_seed(31)
    wn = G.layers.WN(160, 192, kernel_size=5, dilation_rate=1, n_layers=4, p_dropout=0.05).cuda().train()
    b, t = 3, 112
    x0 = torch.randn(b, 192, t, device="cuda")
    lens = torch.tensor([112, 90, 57], device="cuda")
    mask = (torch.arange(t, device="cuda")[None] < lens[:, None]).float()[:, None]
    r = torch.randn(b, 192, t, device="cuda")
    old = convops._WN_NATIVE
    outs = {}
    try:
        for mode in ("off", "fwd", "both"):
            convops._WN_NATIVE = mode
            for p in wn.parameters():
                p.grad = torch.zeros_like(p)
            torch.manual_seed(77)                                   # same dropout masks in every mode
            x = (x0 * mask).clone().requires_grad_(True)
            y = wn(x, mask)
            (y * r).sum().backward()
            torch.cuda.synchronize()
            outs[mode] = (y.detach().clone(), x.grad.clone(), {k: p.grad.clone() for k, p in wn.named_parameters()})
    finally:
        convops._WN_NATIVE = old
    y0, dx0, g0 = outs["off"]
    for mode in ("fwd", "both"):
        y1, dx1, g1 = outs[mode]
        assert_close(y1, y0, what=f"{mode}: y", rtol=1e-6, atol=1e-6)
        assert_close(dx1, dx0, what=f"{mode}: dx", rtol=1e-5, atol=1e-6 * max(1.0, float(dx0.abs().max())))
        for k in g0:
            assert_close(g1[k], g0[k], what=f"{mode}: grad {k}", rtol=2e-4, atol=2e-5 * max(1.0, float(g0[k].abs().max())))


def _torch_encoder(enc, x, x_mask, keep, p):
    """attentions.Encoder.forward in plain torch ops with the dropout keep-masks given (reference attentions.py:63-73,
    204-264, 373-381; relative attention through the package's index-based general path)."""
    import torch.nn.functional as F

    b, hch, t = x.shape
    nh = enc.n_heads
    sizes = [b * nh * t * t, b * hch * t, b * enc.filter_channels * t, b * hch * t]
    scale = 1.0 / (1.0 - p) if p > 0 else 1.0
    pos = 0
    pair = x_mask.unsqueeze(2) * x_mask.unsqueeze(-1)
    ln = lambda v, n: F.layer_norm(v.transpose(1, 2), (hch,), n.gamma, n.beta, n.eps).transpose(1, 2)      # noqa: E731
    for attn, n1, ffn, n2 in zip(enc.attn_layers, enc.norm_layers_1, enc.ffn_layers, enc.norm_layers_2):
        from glow_tts_train import ops as _ops

        ks = []
        raw_attn = None if keep is None else keep[pos: pos + sizes[0]].view(b, nh, t, t).contiguous()
        for n, shape in zip(sizes, [(b, nh, t, t), (b, hch, t), (b, enc.filter_channels, t), (b, hch, t)]):
            ks.append(None if keep is None else keep[pos: pos + n].view(shape).float() * scale)
            pos += n
        x = x * x_mask
        q, k, v = (F.conv1d(x, c.weight, c.bias) for c in (attn.conv_q, attn.conv_k, attn.conv_v))
        # the general path draws its p_attn keep-mask through ops.keep_mask: hand it the executor's decisions
        _ops.keep_mask_inject = (lambda site, shape, pd, _m=raw_attn: _m) if raw_attn is not None else None
        try:
            y, _ = attn._attention_general(q, k, v, pair)
        finally:
            _ops.keep_mask_inject = None
        y = F.conv1d(y, attn.conv_o.weight, attn.conv_o.bias)
        x = ln(x + (y if ks[1] is None else y * ks[1]), n1)
        pad = ffn.kernel_size // 2
        hh = torch.relu(F.conv1d(x * x_mask, ffn.conv_1.weight, ffn.conv_1.bias, padding=pad))
        hh = hh if ks[2] is None else hh * ks[2]
        y = F.conv1d(hh * x_mask, ffn.conv_2.weight, ffn.conv_2.bias, padding=pad) * x_mask
        x = ln(x + (y if ks[3] is None else y * ks[3]), n2)
    return x * x_mask


@pytest.mark.parametrize("b,hch,fch,t,nl,win,p", [(3, 32, 64, 37, 2, 4, 0.0), (2, 192, 768, 160, 2, 4, 0.1), (2, 64, 128, 256, 1, None, 0.1)])
def test_encoder_layer_executor_vs_torch_and_per_op_path(G, b, hch, fch, t, nl, win, p):
    """convops.EncoderLayerFn (a whole transformer layer queued from C: q/k/v with the mask folded in, attention, both
    dropouts of the residual branches inside the LayerNorm kernels, ReLU + dropout as conv epilogue / backward gate) against
    a plain-torch statement of attentions.Encoder with the SAME keep-masks, and (p = 0) against the per-operator path."""
    from glow_tts_train import convops, optimize

    torch.manual_seed(13)
    enc = G.attentions.Encoder(hch, fch, 2, nl, kernel_size=3, p_dropout=p, window_size=win).cuda().train()
    groups = [convops.ConvGroup([a.conv_q, a.conv_k, a.conv_v, a.conv_o, f.conv_1, f.conv_2])
              for a, f in zip(enc.attn_layers, enc.ffn_layers)]
    opt = optimize.Adam(enc.parameters(), scheduler="noam", dim_model=hch)     # flat gradient buffers: in-place gradients
    x0 = torch.randn(b, hch, t, device="cuda")
    lens = torch.tensor([t, max(1, t - 9), max(1, t // 2)][:b], device="cuda")
    mask = (torch.arange(t, device="cuda")[None] < lens[:, None]).float().unsqueeze(1)
    r = torch.randn(b, hch, t, device="cuda")

    def run(native, stack=True):
        convops._WN_NATIVE = "both" if native else "fwd"
        G.attentions._ENC_STACK = stack
        opt.zero_grad()
        for g in groups:
            g.begin()
        torch.manual_seed(99)
        x = x0.clone().requires_grad_(True)
        y = enc(x, mask)
        (y * r).sum().backward()
        convops.flush_groups()
        torch.cuda.synchronize()
        convops._WN_NATIVE = "both"
        G.attentions._ENC_STACK = True
        return y.detach().clone(), x.grad.clone(), {k_: p_.grad.clone() for k_, p_ in enc.named_parameters()}

    calls, stack_calls = [], []
    orig, orig_stack = convops.EncoderLayerFn.forward, convops.EncoderStackFn.forward
    convops.EncoderLayerFn.forward = staticmethod(lambda *a, _o=orig: (calls.append(1), _o(*a))[1])
    convops.EncoderStackFn.forward = staticmethod(lambda *a, _o=orig_stack: (stack_calls.append(1), _o(*a))[1])
    try:
        y1, dx1, g1 = run(True)                              # every layer in ONE autograd node (convops.EncoderStackFn)
        assert (len(calls), len(stack_calls)) == (0, 1), "the stack executor did not run"
        y2, dx2, g2 = run(True, stack=False)                 # one node per layer: the same launches
        assert (len(calls), len(stack_calls)) == (nl, 1), "the layer executor did not run"
    finally:
        convops.EncoderLayerFn.forward = orig
        convops.EncoderStackFn.forward = orig_stack
    assert_close(y2, y1, what="y: layer nodes vs stack node", rtol=1e-6, atol=1e-6)
    assert_close(dx2, dx1, what="dx: layer nodes vs stack node", rtol=1e-5, atol=1e-6 * float(dx1.abs().max()))
    for k_ in g1:
        assert_close(g2[k_], g1[k_], what=f"grad {k_}: layer nodes vs stack node", rtol=2e-4, atol=2e-5 * max(1.0, float(g1[k_].abs().max())))
    # plain torch with the same keep-masks (the executor draws them in ONE generator call at the top of Encoder.forward)
    keep = None
    if p > 0:
        torch.manual_seed(99)
        n_keep = nl * (b * 2 * t * t + 2 * b * hch * t + b * fch * t)
        keep = G.ops.keep_mask((n_keep,), p, "cuda")          # the same generator, the same seed draw
    for p_ in enc.parameters():
        p_.grad = None
    xr = x0.clone().requires_grad_(True)
    yr = _torch_encoder(enc, xr, mask, keep, p)
    (yr * r).sum().backward()
    assert_close(y1, yr, what="y", rtol=2e-4, atol=2e-4)
    assert_close(dx1, xr.grad, what="dx", rtol=2e-3, atol=2e-4 * float(xr.grad.abs().max()))
    gmax = max(float(p_.grad.abs().max()) for p_ in enc.parameters())
    for k_, p_ in enc.named_parameters():
        want = p_.grad       # (floor at 1e-5 of the model's largest gradient: the key bias's gradient is mathematically zero)
        assert_close(g1[k_], want, what=f"grad {k_}", rtol=2e-3, atol=3e-4 * float(want.abs().max()) + 1e-5 * gmax)
    opt._optim.zero_grad()                                   # (re-attach the flat gradient views for the next run)
    if p == 0.0:
        y0, dx0, g0 = run(False)
        assert_close(y1, y0, what="y vs per-op", rtol=1e-5, atol=1e-5)
        assert_close(dx1, dx0, what="dx vs per-op", rtol=1e-4, atol=1e-5 * float(dx0.abs().max()))
        for k_ in g0:
            assert_close(g1[k_], g0[k_], what=f"grad {k_} vs per-op", rtol=2e-4, atol=2e-5 * max(1.0, float(g0[k_].abs().max())))


@pytest.mark.usefixtures("conv_mode")
@pytest.mark.parametrize("b,h,t,blocks,p_drop,sig,gin", [(3, 192, 100, 2, 0.0, False, 0), (2, 192, 64, 2, 0.05, False, 0),
                                                           (2, 48, 37, 3, 0.0, True, 0), (3, 192, 80, 2, 0.05, False, 16),
                                                           (2, 48, 37, 2, 0.0, True, 8), (2, 48, 37, 1, 0.0, True, 0)])
def test_flow_block_executor_matches_per_op_path(G, b, h, t, blocks, p_drop, sig, gin):
    """convops.FlowBlockFn (a whole [ActNorm, InvConvNear, CouplingBlock] block queued from C, one autograd node) against
    the per-operator path (five nodes per block): same kernels in the same order, so outputs agree to rounding of the
    atomics; with dropout both draw the same keep-masks from the same generator state."""
    from glow_tts_train import convops

    torch.manual_seed(77)
    dec = G.models.FlowSpecDecoder(80, h, kernel_size=5, dilation_rate=1, n_blocks=blocks, n_layers=3, p_dropout=p_drop,
                                   n_split=4, n_sqz=2, sigmoid_scale=sig, gin_channels=gin).cuda().train()
    with torch.no_grad():
        for f in dec.flows:
            if hasattr(f, "end"):
                f.end.weight.normal_(0, 0.02)
            if hasattr(f, "logs"):
                f.logs.normal_(0, 0.1)
                f.bias.normal_(0, 0.1)
    g0 = torch.randn(b, gin, 1, device="cuda") if gin else None      # speaker embedding rows (models.py:320-323)
    y0 = torch.randn(b, 80, 2 * t, device="cuda")
    lens = torch.tensor([2 * t, 2 * t - 10, t][:b], device="cuda")
    mask = (torch.arange(2 * t, device="cuda")[None] < lens[:, None]).float().unsqueeze(1)
    r = torch.randn(b, 80, 2 * t, device="cuda")
    s = torch.randn(b, device="cuda")
    res = {}
    used = {}
    orig, orig_stack = convops.FlowBlockFn.forward, convops.FlowStackFn.forward
    # "stack": every block in ONE autograd node (convops.FlowStackFn; not with conditioning rows); "both": one node per block;
    # "fwd": the block executor declines, the per-operator path runs
    # "stack+bwd": the stack node with the opt-in one-launch block boundary of the BACKWARD as well (GLOWTTS_FLOW_BOUNDARY_BWD=1)
    # "stack+half": the stack node's forward as two half-batch chains on two streams (GLOWTTS_HALF_BATCH_FWD=1; even batches)
    for mode in ("stack", "stack+bwd", "stack+half", "both", "fwd"):
        convops._WN_NATIVE = "both" if mode.startswith("stack") else mode
        G.models._FLOW_STACK = mode.startswith("stack")
        bnd_bwd, half_fwd = convops._FLOW_BOUNDARY_BWD, convops._HALF_BATCH_FWD
        convops._FLOW_BOUNDARY_BWD = mode == "stack+bwd"
        convops._HALF_BATCH_FWD = mode == "stack+half"
        calls, stack_calls = [], []
        convops.FlowBlockFn.forward = staticmethod(lambda *a, _o=orig, _c=calls: (_c.append(1), _o(*a))[1])
        convops.FlowStackFn.forward = staticmethod(lambda *a, _o=orig_stack, _c=stack_calls: (_c.append(1), _o(*a))[1])
        try:
            for p in dec.parameters():
                p.grad = torch.zeros_like(p)
            torch.manual_seed(5)
            y = (y0 * mask).clone().requires_grad_(True)
            gg = None if g0 is None else g0.clone().requires_grad_(True)
            z, ld = dec(y, mask, g=gg)
            ((z * r).sum() + (ld * s).sum()).backward()
            convops.flush_groups()
            torch.cuda.synchronize()
        finally:
            convops._WN_NATIVE = "both"
            G.models._FLOW_STACK = True
            convops._FLOW_BOUNDARY_BWD, convops._HALF_BATCH_FWD = bnd_bwd, half_fwd
            convops.FlowBlockFn.forward = orig
            convops.FlowStackFn.forward = orig_stack
        used[mode] = (len(calls), len(stack_calls))
        grads = {k: p.grad.clone() for k, p in dec.named_parameters()}
        if gg is not None:
            grads["<speaker rows g>"] = gg.grad.clone()
        res[mode] = (z.detach().clone(), ld.detach().clone(), y.grad.clone(), grads)
    assert used["both"] == (blocks, 0) and used["fwd"] == (0, 0), used
    assert used["stack"] == used["stack+bwd"] == used["stack+half"] == ((0, 1) if gin == 0 else (blocks, 0)), used   # conditioning rows: one node per block
    if gin == 0:                                         # the two half-batch chains run the same kernels on the same utterances
        assert torch.equal(res["stack+half"][0], res["stack"][0])            # (the log-determinants are sums of float atomics)
        assert_close(res["stack+half"][1], res["stack"][1], what="stack+half: logdet", rtol=1e-6, atol=1e-4)
    if blocks == 1:                                      # a one-block stack makes neither the fused launch nor the stack pack: it
        assert torch.equal(res["stack"][0], res["both"][0])                  # queues the launches of the per-block node
    z0, l0, dx0, g0 = res["fwd"]
    for mode in ("both", "stack", "stack+bwd", "stack+half"):
        z1, l1, dx1, g1 = res[mode]
        assert_close(z1, z0, what=f"{mode}: z", rtol=1e-6, atol=1e-6)
        assert_close(l1, l0, what=f"{mode}: logdet", rtol=1e-6, atol=1e-4)
        assert_close(dx1, dx0, what=f"{mode}: dx", rtol=1e-4, atol=1e-5 * float(dx0.abs().max()))
        for k in g0:
            assert_close(g1[k], g0[k], what=f"{mode}: grad {k}", rtol=2e-4, atol=2e-5 * max(1.0, float(g0[k].abs().max())))


@pytest.mark.usefixtures("conv_mode")
@pytest.mark.parametrize("b,h,t,k,nl,dil,prealloc", [
    (2, 16, 37, 5, 3, 1, False),      # rows not 16-byte aligned (T % 4 != 0): generic kernels
    (3, 48, 52, 3, 2, 2, True),       # dilation 2 (pipe wrw fallback), grads pre-allocated (direct sinks, no two-source)
    (2, 192, 96, 5, 4, 1, True),      # the fast paths: native forward, two-source backward, wgrad un-packing
    (1, 192, 400, 5, 2, 1, True),     # one utterance, full config-2 frame count
    (4, 64, 160, 1, 1, 1, False),     # single layer, 1-tap "k"
])
def test_wn_stack_shapes_vs_oracle(G, b, h, t, k, nl, dil, prealloc):
    """WN stack (reference layers.py:83-162) at shapes that take every kernel / host path, against the oracle (torch CPU)."""
    from oracle import glow_oracle as O

    torch.manual_seed(1000 + b * 7 + h + t + k)
    wn = G.layers.WN(2 * h, h, kernel_size=k, dilation_rate=dil, n_layers=nl, p_dropout=0.0).cuda().train()
    x0 = torch.randn(b, h, t)
    lens = torch.randint(max(1, t // 2), t + 1, (b,))
    lens[0] = t
    mask = (torch.arange(t)[None] < lens[:, None]).float()[:, None]
    r = torch.randn(b, h, t)
    for p in wn.parameters():
        p.grad = torch.zeros_like(p) if prealloc else None
    x = (x0 * mask).cuda().requires_grad_(True)
    y = wn(x, mask.cuda())
    (y * r.cuda()).sum().backward()
    torch.cuda.synchronize()

    sd = {"wn." + k_: v.detach().cpu().clone().requires_grad_(True) for k_, v in wn.state_dict().items()}
    xo = (x0 * mask).clone().requires_grad_(True)
    yo = O.wn(sd, "wn", xo, mask, None, h, nl, dil)
    (yo * r).sum().backward()
    assert_close(y, yo, what="y", rtol=2e-4, atol=2e-5 * max(1.0, float(yo.abs().max())))
    assert_close(x.grad, xo.grad, what="dx", rtol=5e-4, atol=5e-5 * max(1.0, float(xo.grad.abs().max())))
    for name, p in wn.named_parameters():
        want = sd["wn." + name].grad
        assert_close(p.grad, want, what=f"grad {name}", rtol=1e-3, atol=1e-4 * max(1.0, float(want.abs().max())))


@pytest.mark.parametrize("b,t,nl,p_drop", [
    (3, 100, 4, 0.05),     # two frame tiles per utterance, ragged lengths, dropout
    (2, 52, 4, 0.0),       # exactly one tile
    (2, 56, 4, 0.05),      # a second tile of 4 frames
    (1, 400, 4, 0.05),     # the config-2 frame count: 8 tiles
    (2, 60, 3, 0.0),       # three layers
    (2, 24, 1, 0.05),      # one layer (all rows are skip rows)
    (4, 212, 2, 0.05),     # two layers, five tiles
])
def test_wn_layer_resident_forward_matches_per_layer_path_and_oracle(G, b, t, nl, p_drop):
    """csrc/wn_fused.hip (the forward of a whole WN stack in one kernel: reference layers.py:138-162) against the per-layer launch
    sequence it replaces — same keep-masks, `glowtts_wn_fused` flipped — and against the oracle: the stack's output, and through
    the backward every tensor the kernel leaves behind for it (x_{l+1}, acts, tanh / sigmoid): dx and all parameter gradients."""
    from glow_tts_train import convops
    from oracle import glow_oracle as O

    h, k = 192, 5
    before_math = convops.set_conv_math("bf16x6+wrw")
    before_fused = G.hip.wn_fused(None)
    try:
        torch.manual_seed(4000 + 13 * b + t + nl)
        wn = G.layers.WN(2 * h, h, kernel_size=k, dilation_rate=1, n_layers=nl, p_dropout=p_drop).cuda().train()
        with torch.no_grad():
            for p in wn.parameters():
                if p.dim() == 1:
                    p.normal_(0, 0.05)               # non-zero biases
        x0 = torch.randn(b, h, t)
        lens = torch.randint(max(1, t // 2), t + 1, (b,))
        lens[0] = t
        mask = (torch.arange(t)[None] < lens[:, None]).float()[:, None]
        r = torch.randn(b, h, t)
        keep = G.ops.keep_mask((nl, b, 2 * h, t), p_drop, "cuda", "test") if p_drop > 0 else None

        def run(fused):
            G.hip.wn_fused(fused)
            for p in wn.parameters():
                p.grad = torch.zeros_like(p)
            x = (x0 * mask).cuda().requires_grad_(True)
            wn._drop_pre = keep
            y = wn(x, mask.cuda())
            (y * r.cuda()).sum().backward()
            torch.cuda.synchronize()
            return y.detach().clone(), x.grad.clone(), {n: p.grad.clone() for n, p in wn.named_parameters()}

        n0 = G.hip.wn_fused_launches()
        y1, dx1, g1 = run(True)
        n1 = G.hip.wn_fused_launches()
        y0, dx0, g0 = run(False)
        assert n1 == n0 + 1 and G.hip.wn_fused_launches() == n1, "the layer-resident kernel ran exactly when it was switched on"
        assert_close(y1, y0, what="y fused vs per-layer", rtol=1e-5, atol=2e-6 * max(1.0, float(y0.abs().max())))
        assert_close(dx1, dx0, what="dx fused vs per-layer", rtol=1e-4, atol=1e-5 * max(1.0, float(dx0.abs().max())))
        for n in g0:
            assert_close(g1[n], g0[n], what=f"grad {n} fused vs per-layer", rtol=1e-4, atol=1e-5 * max(1.0, float(g0[n].abs().max())))

        sd = {"wn." + k_: v.detach().cpu().clone().requires_grad_(True) for k_, v in wn.state_dict().items()}
        xo = (x0 * mask).clone().requires_grad_(True)
        drop = O.KeepMasks({f"wn.{l}": (keep[l].cpu(), p_drop) for l in range(nl)} if keep is not None else {})
        yo = O.wn(sd, "wn", xo, mask, None, h, nl, 1, drop)
        (yo * r).sum().backward()
        assert_close(y1, yo, what="y", rtol=2e-4, atol=2e-5 * max(1.0, float(yo.abs().max())))
        assert_close(dx1, xo.grad, what="dx", rtol=5e-4, atol=5e-5 * max(1.0, float(xo.grad.abs().max())))
        for name, p in wn.named_parameters():
            want = sd["wn." + name].grad
            assert_close(g1[name], want, what=f"grad {name}", rtol=1e-3, atol=1e-4 * max(1.0, float(want.abs().max())))
    finally:
        G.hip.wn_fused(before_fused)
        convops.set_conv_math(before_math)


def test_multi_stream_step_matches_single_stream_step(G):
    """train_batch overlaps the text encoder, the weight-gradient kernels and the dx chain on three streams.  Three optimisation
    steps with the overlap must leave the same parameters as three steps with everything on one stream (GLOWTTS_SIDE_STREAM=0);
    only the order of float atomics differs.  Production widths, so the kernels are long enough for a missing dependency
    or a recycled buffer to show."""
    import os

    from glow_tts_train.train import train_batch

    def run(side):
        old = os.environ.get("GLOWTTS_SIDE_STREAM")
        os.environ["GLOWTTS_SIDE_STREAM"] = "1" if side else "0"
        try:
            torch.manual_seed(77)
            model = G.models.FlowGenerator(n_vocab=148, hidden_channels=192, filter_channels=768, filter_channels_dp=256,
                                           out_channels=80, kernel_size=3, n_heads=2, n_layers_enc=3, p_dropout=0.0,
                                           n_blocks_dec=4, kernel_size_dec=5, dilation_rate=1, n_block_layers=4,
                                           p_dropout_dec=0.0, n_split=4, n_sqz=2, window_size=4, mean_only=True,
                                           prenet=True).cuda().train()
            for m in model.modules():
                if isinstance(m, torch.nn.Dropout):
                    m.p = 0.0
            with torch.no_grad():
                for f in model.decoder.flows:
                    if hasattr(f, "end"):
                        f.end.weight.normal_(0, 0.01)
            opt = G.optimize.Adam(model.parameters(), scheduler="noam", dim_model=192, warmup_steps=4000, lr=1.0,
                                  betas=(0.9, 0.98), eps=1e-9)
            g = torch.Generator().manual_seed(5)
            b, tx, ty = 8, 48, 240
            x = torch.randint(1, 148, (b, tx), generator=g).cuda()
            xl = torch.linspace(tx, tx // 2, b).long().cuda()
            y = torch.randn(b, 80, ty, generator=g).cuda()
            yl = torch.linspace(ty, ty // 2, b).long().cuda()
            losses = [float(train_batch(model, opt, (x, xl, y, yl, None), 5.0)) for _ in range(3)]
            torch.cuda.synchronize()
            return losses, opt._optim.flat_p.detach().clone(), opt._optim.flat_g.detach().clone()
        finally:
            if old is None:
                os.environ.pop("GLOWTTS_SIDE_STREAM", None)
            else:
                os.environ["GLOWTTS_SIDE_STREAM"] = old

    l1, p1, g1 = run(True)
    l0, p0, g0 = run(False)
    assert all(abs(a - b) <= 1e-4 * max(1.0, abs(b)) for a, b in zip(l1, l0)), (l1, l0)
    assert_close(g1, g0, what="last step's gradients", rtol=1e-3, atol=2e-5 * float(g0.abs().max()))   # (atomics-order noise is ~5e-7; a race showed up as 1e-4: DESIGN.md lesson 12)
    # Adam's first steps move every weight by ~lr regardless of the gradient's size, so compare the update, not the weight
    assert float((p1 - p0).abs().max()) <= 2e-3 * float(p0.abs().max()) + 1e-6


def test_graphed_train_step_matches_eager(G):
    """hipGraph replay of the whole step == eager launches (same kernels, same order, same on-device schedule)."""
    from glow_tts_train.train import GraphedTrainStep, train_batch
    from oracle import glow_oracle as O

    hp = O.HParams(n_vocab=40, hidden_channels=32, filter_channels=64, filter_channels_dp=32, n_layers_enc=1,
                   n_blocks_dec=2, n_block_layers=2)
    torch.manual_seed(3)
    b, tx, ty = 2, 8, 32
    x = torch.randint(1, 40, (b, tx)).cuda()
    xl = torch.tensor([8, 5]).cuda()
    y = torch.randn(b, 80, ty).cuda()
    yl = torch.tensor([32, 20]).cuda()
    batch = (x, xl, y, yl, None)
    losses = {}
    finals = {}
    for mode in ("eager", "graph"):
        torch.manual_seed(11)                      # _oracle_pair draws the coupling end-conv weights from the global RNG
        sd, model = _oracle_pair(G, hp, seed=9)
        opt = G.optimize.Adam(model.parameters(), scheduler="noam", dim_model=32, warmup_steps=4000, lr=1.0)
        if mode == "eager":
            ls = [float(train_batch(model, opt, batch, 5.0)) for _ in range(5)]
        else:
            g = GraphedTrainStep(model, opt, 5.0, batch, warmup=2)        # 2 warm-up steps are real optimisation steps
            ls = [None, None] + [float(g()) for _ in range(3)]
            extra = float(train_batch(model, opt, batch, 5.0))             # eager launches still work after a capture
            assert extra < ls[-1] and opt.step_num == 7
            opt.step_num -= 1
            opt._optim.dev_state[:2] -= 1
        losses[mode] = ls
        assert opt.step_num == 6 and float(opt._optim.dev_state[1]) == 6.0
    for a, e in zip(losses["graph"][2:], losses["eager"][2:]):
        assert abs(a - e) <= 2e-4 * abs(e), (losses)
    # (the graph variant made one extra eager step above; compare the trajectories, not the end state)


def test_actnorm_invconv_bwd_is_stable_next_to_the_weight_gradient_kernel(G):
    """Regression (DESIGN.md lesson 12): the fused ActNorm + InvConv backward run NEXT TO the bf16-plane 5-tap weight-gradient
    kernel (second stream, co-resident on the CUs) returned wrong matrix-gradient partials in a few percent of its launches
    while its accumulators were packed-fp32 register pairs; alone it never did.  The library is built without packed-fp32 VALU
    math since; results must repeat to the rounding of the atomics (shape with a partially filled last wave, the worst case)."""
    from glow_tts_train import _hip
    from glow_tts_train._hip import call, ptr

    B, C, T, H = 8, 160, 64, 192
    torch.manual_seed(0)
    x, dz = torch.randn(B, C, T, device="cuda"), torch.randn(B, C, T, device="cuda")
    m = torch.ones(B, T, device="cuda")
    logs, bias = torch.randn(C, device="cuda") * 0.1, torch.randn(C, device="cuda") * 0.1
    w = torch.linalg.qr(torch.randn(4, 4))[0].cuda().contiguous()
    winv = torch.linalg.inv(w).contiguous()
    xlen, dld = m.sum(1), torch.randn(B, device="cuda")
    dx = torch.empty_like(x)
    xw, d2 = torch.randn(B, H, 120, device="cuda"), torch.randn(B, 2 * H, 120, device="cuda")
    dwp5 = torch.zeros(5, H, 2 * H, device="cuda")
    side = torch.cuda.Stream()
    before = _hip.conv_math("bf16x6+wrw")
    try:
        ref, worst = None, 0.0
        for _ in range(120):
            dlogs, dbias, dw = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda"), torch.zeros(16, device="cuda")
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                for _ in range(4):
                    call("glowtts_conv_wrw", ptr(xw), xw.stride(0), ptr(d2), d2.stride(0), None, None, ptr(dwp5), None, B, H, 2 * H,
                         120, 5, 1, 2)
            call("glowtts_actnorm_invconv_bwd", ptr(x), ptr(m), ptr(logs), ptr(bias), ptr(w), ptr(winv), ptr(dz), ptr(dld), ptr(xlen),
                 ptr(dx), ptr(dlogs), ptr(dbias), ptr(dw), B, C, T, 4)
            torch.cuda.synchronize()
            got = torch.cat([dw, dlogs, dbias])
            if ref is None:
                ref = got.clone()
            worst = max(worst, float((got - ref).abs().max() / ref.abs().max()))
    finally:
        _hip.conv_math(before)
    assert worst < 5e-6, worst


@pytest.mark.parametrize("io", [False, "all"])
def test_first_step_gradients_repeat_across_multi_stream_runs(G, io):
    """The gradients of ONE step from identical parameters, three times with the side streams on and once without: every
    element within 5e-6 of the largest gradient (float atomics land in a different order: ~5e-7).  A kernel that goes wrong
    only next to another stream's kernels (DESIGN.md lesson 12) shows up here as 1e-4."""
    from glow_tts_train.train import train_batch

    def run(side):
        old = os.environ.get("GLOWTTS_SIDE_STREAM")
        os.environ["GLOWTTS_SIDE_STREAM"] = "1" if side else "0"
        try:
            torch.manual_seed(77)
            model = G.models.FlowGenerator(n_vocab=148, hidden_channels=192, filter_channels=768, filter_channels_dp=256,
                                           out_channels=80, kernel_size=3, n_heads=2, n_layers_enc=3, p_dropout=0.0,
                                           n_blocks_dec=4, kernel_size_dec=5, dilation_rate=1, n_block_layers=4,
                                           p_dropout_dec=0.0, n_split=4, n_sqz=2, window_size=4, mean_only=True,
                                           prenet=True).cuda().train()
            for m in model.modules():
                if isinstance(m, torch.nn.Dropout):
                    m.p = 0.0
            with torch.no_grad():
                for f in model.decoder.flows:
                    if hasattr(f, "end"):
                        f.end.weight.normal_(0, 0.01)
            model.decoder.io_bf16 = io                   # (bf16 tensors in HBM: the `_io` kernels)
            opt = G.optimize.Adam(model.parameters(), scheduler="noam", dim_model=192, warmup_steps=4000, lr=1.0,
                                  betas=(0.9, 0.98), eps=1e-9)
            g = torch.Generator().manual_seed(5)
            b, tx, ty = 8, 48, 248                       # T' = 124: a partially filled last wave in the flow kernels
            x = torch.randint(1, 148, (b, tx), generator=g).cuda()
            xl = torch.linspace(tx, tx // 2, b).long().cuda()
            y = torch.randn(b, 80, ty, generator=g).cuda()
            yl = torch.linspace(ty, ty // 2, b).long().cuda()
            train_batch(model, opt, (x, xl, y, yl, None), 5.0)
            torch.cuda.synchronize()
            return opt._optim.flat_g.detach().clone()
        finally:
            if old is None:
                os.environ.pop("GLOWTTS_SIDE_STREAM", None)
            else:
                os.environ["GLOWTTS_SIDE_STREAM"] = old

    ref = run(False)
    gmax = float(ref.abs().max())
    for i in range(3):
        got = run(True)
        worst = float((got - ref).abs().max()) / gmax
        assert worst < 5e-6, (i, worst)


# ---- several convolutions per launch on 16-row tiles (csrc/packw.hip): weight norm + both packings + bf16 planes, and the
# backward through the weight norm, against torch.nn.utils.weight_norm semantics (reference layers.py:113,125,135)
_PACK_SHAPES = [(384, 192, 5, True), (384, 192, 1, True), (192, 80, 1, False), (160, 192, 1, False), (80, 192, 1, True),
                (1, 256, 1, False), (256, 1, 1, False), (768, 192, 3, False), (192, 768, 3, True), (40, 24, 2, True), (50, 70, 3, True)]


def _pack_reference(v, g):
    w = v if g is None else v * (g / v.flatten(1).norm(dim=1).view(-1, 1, 1))
    co, ci, k = v.shape
    gi, go = (ci + 15) // 16, (co + 15) // 16
    wf = torch.zeros(k, gi * 16, co, dtype=w.dtype, device=w.device)
    wf[:, :ci] = w.permute(2, 1, 0)                                  # [tap][c][o]
    wf = wf.view(k, gi, 16, co).permute(0, 1, 3, 2).contiguous()     # [tap][c/16][o][c%16]
    wb = torch.zeros(k, go * 16, ci, dtype=w.dtype, device=w.device)
    wb[:, :co] = w.flip(2).permute(2, 0, 1)                          # [taps-1-tap][o][c]
    wb = wb.view(k, go, 16, ci).permute(0, 1, 3, 2).contiguous()     # [tap'][o/16][c][o%16]
    return wf, wb


def test_pack_and_unpack_tile_kernels_vs_torch(G):
    call, ptr = G.hip.call, G.hip.ptr
    torch.manual_seed(3)
    dev = "cuda"
    vs = [torch.randn(co, ci, k, device=dev) * 0.2 for co, ci, k, _ in _PACK_SHAPES]
    gs = [(torch.rand(co, 1, 1, device=dev) + 0.5) if wn else None for co, ci, k, wn in _PACK_SHAPES]
    sizes = [(k * ((ci + 15) // 16) * co * 16, k * ((co + 15) // 16) * ci * 16) for co, ci, k, _ in _PACK_SHAPES]
    arena = torch.zeros(sum(a + b for a, b in sizes), device=dev)
    planes = torch.zeros(3 * arena.numel(), device=dev, dtype=torch.int16)
    invs = [torch.zeros(co, device=dev) for co, _, _, _ in _PACK_SHAPES]
    desc, views, cur, rows = [], [], 0, [0]
    for (co, ci, k, wn), v, g, inv, (sa, sb) in zip(_PACK_SHAPES, vs, gs, invs, sizes):
        f, b = arena[cur: cur + sa], arena[cur + sa: cur + sa + sb]
        cur += sa + sb
        views.append((f, b))
        desc.append([v.data_ptr(), 0 if g is None else g.data_ptr(), f.data_ptr(), b.data_ptr(), inv.data_ptr() if wn else 0, co, ci, k])
        rows.append(rows[-1] + co)
    desc_t = torch.tensor(desc, dtype=torch.int64, device=dev)
    prefix = torch.tensor(rows, dtype=torch.int32, device=dev)
    call("glowtts_pack_weight_planes_multi", ptr(desc_t), ptr(prefix), len(desc), rows[-1], ptr(arena), arena.numel(), ptr(planes))
    torch.cuda.synchronize()
    for (co, ci, k, wn), v, g, inv, (f, b) in zip(_PACK_SHAPES, vs, gs, invs, views):
        wf, wb = _pack_reference(v.double(), None if g is None else g.double())
        assert_close(f.view_as(wf), wf.float(), rtol=2e-6, atol=1e-7, what=f"wp_f {co, ci, k}")
        assert_close(b.view_as(wb), wb.float(), rtol=2e-6, atol=1e-7, what=f"wp_b {co, ci, k}")
        if wn:
            assert_close(inv, (1.0 / v.double().flatten(1).norm(dim=1)).float(), rtol=2e-6, atol=0, what="inv_norm")
    # the planes are the exact three-way split of the packed fp32 values: h + m + l == w bit for bit, h = bf16(w)
    pl = planes.view(3, -1).to(torch.int32).bitwise_and(0xFFFF).bitwise_left_shift(16).view(torch.float32)
    assert torch.equal(pl[0] + pl[1] + pl[2], arena), "planes do not add up to the packed weights"
    assert torch.equal(pl[0], arena.to(torch.bfloat16).float()), "plane 0 is not the nearest bf16"
    # the plain entry point writes the same fp32 packings
    arena2 = arena.clone().zero_()
    desc2 = desc_t.clone()
    desc2[:, 2] += arena2.data_ptr() - arena.data_ptr()
    desc2[:, 3] += arena2.data_ptr() - arena.data_ptr()
    call("glowtts_pack_weight_multi", ptr(desc2), ptr(prefix), len(desc), rows[-1])
    assert torch.equal(arena2, arena)

    # ---- backward: packed gradient [tap][c][o] -> dv (+=), dg (+=)
    dws = [torch.randn(k, ci, co, device=dev) for co, ci, k, _ in _PACK_SHAPES]
    dvs = [torch.randn_like(v) for v in vs]
    dgs = [None if g is None else torch.randn_like(g) for g in gs]
    dv0 = [d.clone() for d in dvs]
    dg0 = [None if d is None else d.clone() for d in dgs]
    ud = [[dw.data_ptr(), v.data_ptr(), 0 if g is None else g.data_ptr(), inv.data_ptr() if g is not None else 0, dv.data_ptr(),
           0 if dg is None else dg.data_ptr(), co, ci, k]
          for (co, ci, k, _), dw, v, g, inv, dv, dg in zip(_PACK_SHAPES, dws, vs, gs, invs, dvs, dgs)]
    ud_t = torch.tensor(ud, dtype=torch.int64, device=dev)
    call("glowtts_unpack_weight_grad_multi", ptr(ud_t), ptr(prefix), len(ud), rows[-1])
    torch.cuda.synchronize()
    for (co, ci, k, wn), dw, v, g, dv, dg, a0, b0 in zip(_PACK_SHAPES, dws, vs, gs, dvs, dgs, dv0, dg0):
        v64 = v.double().requires_grad_(True)
        g64 = None if g is None else g.double().requires_grad_(True)
        w = v64 if g64 is None else v64 * (g64 / v64.flatten(1).norm(dim=1).view(-1, 1, 1))
        (w * dw.double().permute(2, 1, 0)).sum().backward()
        assert_close(dv - a0, v64.grad.float(), rtol=1e-5, atol=2e-6 * float(v64.grad.abs().max()), what=f"dv {co, ci, k}")
        if wn:
            assert_close(dg - b0, g64.grad.float(), rtol=1e-5, atol=2e-6 * float(g64.grad.abs().max()), what=f"dg {co, ci, k}")


# ---- several weight gradients of one shape in one launch (glowtts_conv_wrw_batch) against one launch per problem
@pytest.mark.parametrize("taps,two,masked,n", [(5, False, False, 4), (1, True, False, 3), (1, False, True, 3), (3, False, False, 5)])
def test_conv_wrw_batch_matches_single_launches(G, conv_mode, taps, two, masked, n):
    import ctypes

    call, ptr = G.hip.call, G.hip.ptr
    torch.manual_seed(taps + n)
    b, k, m, t = 6, 192, 384, 120
    keep = []

    def parr(ts):
        a = (ctypes.c_void_p * len(ts))(*[x.data_ptr() for x in ts])
        keep.append(a)
        return ctypes.addressof(a)

    xs = [torch.randn(b, k, t, device="cuda") for _ in range(n)]
    ds = [torch.randn(b, m // 2 if two else m, t, device="cuda") for _ in range(n)]
    d2 = [torch.randn(b, m // 2, t, device="cuda") for _ in range(n)] if two else None
    lens = torch.linspace(t, t // 2, b).long()
    mask = (torch.arange(t)[None] < lens[:, None]).float().cuda() if masked else None
    ref = [torch.zeros(taps, k, m, device="cuda") for _ in range(n)]
    out = [torch.zeros(taps, k, m, device="cuda") for _ in range(n)]
    rb = [torch.zeros(m, device="cuda") for _ in range(n)]
    ob = [torch.zeros(m, device="cuda") for _ in range(n)]
    pad = (taps - 1) // 2
    for q in range(n):
        if two:
            call("glowtts_conv_wrw2", ptr(xs[q]), xs[q].stride(0), ptr(ds[q]), ds[q].stride(0), ptr(d2[q]), d2[q].stride(0), m // 2,
                 ptr(ref[q]), ptr(rb[q]), b, k, m, t, taps, 1, pad)
        else:
            call("glowtts_conv_wrw", ptr(xs[q]), xs[q].stride(0), ptr(ds[q]), ds[q].stride(0), ptr(mask) if masked else None,
                 ptr(mask) if masked else None, ptr(ref[q]), ptr(rb[q]), b, k, m, t, taps, 1, pad)
    call("glowtts_conv_wrw_batch", n, parr(xs), xs[0].stride(0), parr(ds), ds[0].stride(0), parr(d2) if two else None,
         d2[0].stride(0) if two else 0, m // 2 if two else 0, ptr(mask) if masked else None, ptr(mask) if masked else None, parr(out),
         parr(ob), b, k, m, t, taps, 1, pad)
    torch.cuda.synchronize()
    for q in range(n):          # same kernels, same arithmetic: only the order of the split-K atomics differs
        assert_close(out[q], ref[q], rtol=0, atol=2e-6 * float(ref[q].abs().max()), what=f"dW of problem {q}")
        assert_close(ob[q], rb[q], rtol=0, atol=2e-6 * float(rb[q].abs().max()), what=f"dbias of problem {q}")
    xd = xs[0].double() * (mask[:, None].double() if masked else 1.0)
    dd = (torch.cat([ds[0], d2[0]], 1) if two else ds[0]).double() * (mask[:, None].double() if masked else 1.0)
    want = torch.nn.grad.conv1d_weight(xd, (m, k, taps), dd, padding=pad).permute(2, 1, 0)
    assert rel_err(out[0], want.float()) < 2e-5


def test_keep_mask_kernel_statistics_and_repeatability(G):
    """glowtts_keep_mask: Bernoulli(1 - p) bytes from Philox4x32-7 — right rate, no structure across bytes of a group, the same
    mask for the same seed, another one for another seed, any length."""
    call, ptr = G.hip.call, G.hip.ptr
    n = 8 * 1000 * 1000 + 5
    for p in (0.05, 0.1, 0.5):
        a = torch.empty(n, device="cuda", dtype=torch.uint8)
        b = torch.full((n + 8,), 7, device="cuda", dtype=torch.uint8)
        call("glowtts_keep_mask", ptr(a), n, 1234567, p)
        call("glowtts_keep_mask", ptr(b), n, 1234567, p)
        assert torch.equal(a, b[:n]) and bool((b[n:] == 7).all()), "same seed, same mask; nothing written past n"
        assert int(a.max()) == 1 and int(a.min()) == 0
        keep = float(a.float().mean())
        sigma = (p * (1 - p) / n) ** 0.5
        assert abs(keep - (1 - p)) < 5 * sigma + 2e-5, (p, keep)
        by_pos = a[: n - 5].view(-1, 8).float().mean(0)                       # each of the 8 bytes a thread writes
        assert float((by_pos - (1 - p)).abs().max()) < 6 * sigma * 8 ** 0.5 + 2e-5
        x = a[: n - 5].view(-1, 8).float() - (1 - p)
        corr = (x.t() @ x) / x.shape[0] / (p * (1 - p))                      # correlation between byte positions
        off = corr - torch.diag(torch.diag(corr))
        assert float(off.abs().max()) < 6e-3 and float((torch.diag(corr) - 1).abs().max()) < 3e-2   # (1e6 samples: sigma 1e-3)
        c = torch.empty(n, device="cuda", dtype=torch.uint8)
        call("glowtts_keep_mask", ptr(c), n, 1234568, p)
        agree = float((a == c).float().mean())
        assert abs(agree - ((1 - p) ** 2 + p ** 2)) < 2e-3, "another seed: an independent mask"
    m = G.ops.keep_mask((3, 5, 7), 0.25, "cuda")
    assert m.shape == (3, 5, 7) and m.dtype == torch.uint8


@pytest.mark.parametrize("b,c,h,t,ns,sig", [(3, 160, 192, 400, 4, 0), (2, 160, 192, 52, 4, 1), (2, 64, 96, 36, 2, 0), (1, 192, 192, 128, 4, 0)])
def test_flow_boundary_kernel_equals_its_three_launches(G, b, c, h, t, ns, sig):
    """csrc/flow_boundary.hip: end conv(k) + coupling(k) + ActNorm / InvConv(k + 1) + start conv(k + 1) in one launch against the
    three launches it replaces (1x1 conv, glowtts_coupling_actnorm_invconv_fwd, 1x1 conv with masked output): the matrix products
    are the same fp32 MFMAs in the same order, so out / y / h0 must agree bit for bit; the log-determinants to fp32 summation order.
    Ragged lengths, a last frame tile of 4 / 16 / 20 frames, channel counts that leave row tiles and k groups partly empty."""
    from glow_tts_train._hip import call

    P = lambda x: x.data_ptr()                                             # noqa: E731
    torch.manual_seed(c + t)
    f = lambda *s: torch.randn(*s, device="cuda")                          # noqa: E731
    lens = torch.tensor([t, max(1, t - 7), max(1, t // 2)][:b], device="cuda")
    mask = (torch.arange(t, device="cuda")[None] < lens[:, None]).float().contiguous()
    x_len = lens.float()
    skip, y_prev = f(b, h, t) * mask[:, None], f(b, c, t) * mask[:, None]
    logs, bias, w = f(c) * 0.1, f(c) * 0.1, torch.linalg.qr(f(ns, ns))[0].contiguous()
    if float(torch.det(w)) < 0:                                            # (layers.py:232-234: the reference's init does the same)
        w[:, 0] = -w[:, 0]
    w_inv, logdet_w = torch.empty(ns * ns + 1, device="cuda"), None
    call("glowtts_invconv_prepare", P(w), P(w_inv), P(w_inv) + 4 * ns * ns, ns)
    logdet_w = w_inv[ns * ns:]
    gh, gs = (h + 15) // 16, (c // 2 + 15) // 16
    # packed weights [G][M][16] with zeros at the k positions beyond the channel count, as glowtts_pack_weight* leaves them
    wp_end = torch.zeros(gh, c, 16, device="cuda")
    wp_end.view(gh, c, 16).copy_((f(gh, c, 16) * 0.05) * (torch.arange(gh * 16, device="cuda").view(gh, 1, 16) < h))
    wp_start = torch.zeros(gs, h, 16, device="cuda")
    wp_start.copy_((f(gs, h, 16) * 0.05) * (torch.arange(gs * 16, device="cuda").view(gs, 1, 16) < c // 2))
    b_end, b_start = f(c) * 0.1, f(h) * 0.1
    got = [torch.full((b, c, t), float("nan"), device="cuda"), torch.full((b, c, t), float("nan"), device="cuda"),
           torch.full((b, h, t), float("nan"), device="cuda"), torch.ones(b, device="cuda"), torch.full((b,), float("nan"), device="cuda")]
    want = [x.clone() for x in got]
    call("glowtts_flow_boundary_fwd", P(skip), P(wp_end), P(b_end), P(y_prev), P(mask), P(logs), P(bias), P(w), P(logdet_w), P(x_len),
         P(wp_start), P(b_start), P(got[0]), P(got[1]), P(got[2]), P(got[3]), P(got[4]), b, c, h, t, ns, sig)
    call("glowtts_conv_fwd", P(skip), h * t, P(wp_end), P(b_end), None, None, 0, P(want[0]), c * t, b, h, c, t, 1, 1, 0, 0, 0, 0)
    call("glowtts_coupling_actnorm_invconv_fwd", P(y_prev), P(want[0]), P(mask), P(logs), P(bias), P(w), P(logdet_w), P(x_len),
         P(want[1]), P(want[3]), P(want[4]), b, c, t, ns, sig)
    call("glowtts_conv_fwd", P(want[1]), c * t, P(wp_start), P(b_start), P(mask), None, 0, P(want[2]), h * t, b, c // 2, h, t, 1, 1, 0,
         0, 1, 0)
    torch.cuda.synchronize()
    for name, a, e in zip(("out", "y", "h0"), got, want):
        assert torch.equal(a, e), (name, float((a - e).abs().max()))
    assert_close(got[3], want[3], what="logdet_prev", rtol=1e-5, atol=1e-4 * max(1.0, float(want[3].abs().max())))
    assert_close(got[4], want[4], what="logdet", rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("b,c,h,t,ns,sig,mask_dskip", [(3, 160, 192, 400, 4, 0, 1), (2, 160, 192, 52, 4, 1, 0), (2, 64, 96, 36, 2, 0, 1),
                                                        (1, 192, 192, 128, 4, 0, 1)])
def test_flow_boundary_backward_kernel_equals_its_three_launches(G, b, c, h, t, ns, sig, mask_dskip):
    """csrc/flow_boundary.hip backwards: start conv backward-data(k + 1) + ActNorm / InvConv backward(k + 1) + coupling backward(k) +
    end conv backward-data(k) in one launch (+ the small reduction of the parameter-gradient partials) against the three launches it
    replaces: dy, dout, dskip bit for bit (same MFMA products in the same order, same element-wise arithmetic); dlogs / dbias / dW
    to fp32 summation order."""
    from glow_tts_train._hip import call

    P = lambda x: x.data_ptr()                                             # noqa: E731
    torch.manual_seed(c + 3 * t)
    f = lambda *s: torch.randn(*s, device="cuda")                          # noqa: E731
    lens = torch.tensor([t, max(1, t - 7), max(1, t // 2)][:b], device="cuda")
    mask = (torch.arange(t, device="cuda")[None] < lens[:, None]).float().contiguous()
    x_len = lens.float()
    dx_wn, dy_next = f(b, h, t), f(b, c, t)
    y_prev, out_prev = f(b, c, t) * mask[:, None], f(b, c, t) * 0.3
    logs, bias, w = f(c) * 0.1, f(c) * 0.1, torch.linalg.qr(f(ns, ns))[0].contiguous()
    if float(torch.det(w)) < 0:
        w[:, 0] = -w[:, 0]
    w_inv = torch.empty(ns * ns + 1, device="cuda")
    call("glowtts_invconv_prepare", P(w), P(w_inv), P(w_inv) + 4 * ns * ns, ns)
    dlogdet = f(b)
    gh, gc = (h + 15) // 16, (c + 15) // 16
    wb_start = (f(gh, c // 2, 16) * 0.05) * (torch.arange(gh * 16, device="cuda").view(gh, 1, 16) < h)      # [G(H)][C/2][16]
    wb_end = (f(gc, h, 16) * 0.05) * (torch.arange(gc * 16, device="cuda").view(gc, 1, 16) < c)             # [G(C)][H][16]
    wb_start, wb_end = wb_start.contiguous(), wb_end.contiguous()
    nan = float("nan")
    got = [torch.full((b, c, t), nan, device="cuda"), torch.full((b, c, t), nan, device="cuda"), torch.full((b, h, t), nan, device="cuda")]
    ggrad = [torch.zeros(c, device="cuda"), torch.zeros(c, device="cuda"), torch.zeros(ns, ns, device="cuda")]
    want = [x.clone() for x in got]
    wgrad = [x.clone() for x in ggrad]
    n_part = b * ((t + 31) // 32) * (c // ns) * (2 * ns + ns * ns)
    part = torch.full((n_part,), nan, device="cuda")
    call("glowtts_flow_boundary_bwd", P(dx_wn), P(wb_start), P(dy_next), P(y_prev), P(out_prev), P(mask), P(logs), P(bias), P(w),
         P(dlogdet), P(wb_end), P(got[0]), P(got[1]), P(got[2]), P(part), b, c, h, t, ns, sig, mask_dskip)
    call("glowtts_flow_boundary_bwd_reduce", P(part), P(w_inv), P(dlogdet), P(x_len), P(ggrad[0]), P(ggrad[1]), P(ggrad[2]), b, c, t, ns)
    # the three launches: dy_next[:, :C/2] += W_start^T (dx_wn mask) ; the fused flow backward ; dskip = W_end^T dout [mask]
    dyf = dy_next.clone()
    call("glowtts_conv_fwd", P(dx_wn), h * t, P(wb_start), None, P(mask), P(dyf), c * t, P(dyf), c * t, b, h, c // 2, t, 1, 1, 0, 1, 0, 0)
    call("glowtts_coupling_actnorm_invconv_bwd", P(y_prev), P(out_prev), P(mask), P(logs), P(bias), P(w), P(w_inv), P(dyf), P(dlogdet),
         P(x_len), P(want[0]), P(want[1]), P(wgrad[0]), P(wgrad[1]), P(wgrad[2]), b, c, t, ns, sig)
    call("glowtts_conv_fwd", P(want[1]), c * t, P(wb_end), None, P(mask) if mask_dskip else None, None, 0, P(want[2]), h * t, b, c, h, t,
         1, 1, 0, 0, mask_dskip, 0)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(part).any()), "a partial was left unwritten"
    for name, a, e in zip(("dy", "dout", "dskip"), got, want):
        assert torch.equal(a, e), (name, float((a - e).abs().max()))
    for name, a, e in zip(("dlogs", "dbias", "dw"), ggrad, wgrad):
        assert_close(a, e, what=name, rtol=2e-4, atol=2e-4 * max(1.0, float(e.abs().max())))
