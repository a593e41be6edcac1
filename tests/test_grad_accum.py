"""GPU tests (-m gpu) of gradient accumulation: the scale + norm + clamp kernel, train.train_batches against per-micro-batch
runs and against the CPU oracle, the once-per-update weight packing, and the public edges (accum_steps, tail groups).

Tolerances are the project's own: the per-tensor gradient criterion `5e-3 max|g_tensor| + 1e-5 max|g_model|` and the
`0.05 lr0` rule for a first Adam update on large-gradient elements (tests/test_hip_parity.py, small-config step test)."""
import types

import pytest
import torch

from helpers import assert_close

pytestmark = pytest.mark.gpu

CLIP = 5.0
# (b, t_text, t_mel, text lengths, mel lengths, speakers): three micro-batches of different shapes, ragged inside
MICRO = [
    (4, 30, 160, [30, 25, 17, 9], [160, 140, 101, 48], [0, 3, 1, 2]),
    (3, 22, 104, [22, 15, 8], [104, 77, 40], [2, 0, 3]),
    (2, 12, 56, [12, 7], [56, 33], [1, 2]),
]


@pytest.fixture(scope="module")
def G():
    from glow_tts_train import _hip, convops, models, ops, optimize, train, utils

    _hip.load()
    return types.SimpleNamespace(hip=_hip, convops=convops, models=models, ops=ops, optimize=optimize, train=train, utils=utils)


@pytest.fixture(params=["fp32", "bf16x6+wrw"])
def conv_mode(request):
    """Both arithmetics of the WN-stack convolutions, as tests/test_hip_parity.py's fixture of the same name."""
    from glow_tts_train import convops

    before = convops.set_conv_math(request.param)
    yield request.param
    convops.set_conv_math(before)


@pytest.fixture(scope="module")
def small():
    """The small multi-speaker config of test_full_step_vs_oracle_small_config: hyper-parameters, one state dict, the batches."""
    from oracle import glow_oracle as O

    hp = O.HParams(n_vocab=60, hidden_channels=64, filter_channels=128, filter_channels_dp=64, n_layers_enc=2,
                   n_blocks_dec=3, n_block_layers=2, n_speakers=4, gin_channels=16, mean_only=False)
    sd = O.init_state_dict(hp, seed=5)
    gen = torch.Generator().manual_seed(1)
    for k in list(sd):
        if k.endswith(".end.weight"):
            sd[k] = 0.05 * torch.randn(sd[k].shape, generator=gen)
    batches = []
    for b, tx, ty, xl, yl, spk in MICRO:
        xl, yl = torch.tensor(xl), torch.tensor(yl)
        x = torch.randint(1, 60, (b, tx), generator=gen) * (torch.arange(tx)[None] < xl[:, None])
        y = torch.randn(b, 80, ty, generator=gen) * (torch.arange(ty)[None, None] < yl[:, None, None])
        batches.append((x, xl, y, yl, torch.tensor(spk)))
    return types.SimpleNamespace(hp=hp, sd=sd, batches=batches)


def _model(G, small):
    hp = small.hp
    m = G.models.FlowGenerator(
        n_vocab=hp.n_vocab, hidden_channels=hp.hidden_channels, filter_channels=hp.filter_channels,
        filter_channels_dp=hp.filter_channels_dp, out_channels=hp.out_channels, kernel_size=hp.kernel_size,
        n_heads=hp.n_heads, n_layers_enc=hp.n_layers_enc, p_dropout=0.0, n_blocks_dec=hp.n_blocks_dec,
        kernel_size_dec=hp.kernel_size_dec, dilation_rate=hp.dilation_rate, n_block_layers=hp.n_block_layers,
        p_dropout_dec=0.0, n_speakers=hp.n_speakers, gin_channels=hp.gin_channels, n_split=hp.n_split, n_sqz=hp.n_sqz,
        sigmoid_scale=hp.sigmoid_scale, window_size=hp.window_size, mean_only=hp.mean_only, prenet=hp.prenet)
    m.load_state_dict(small.sd)
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    m = m.cuda().train()
    opt = G.optimize.Adam(m.parameters(), scheduler="noam", dim_model=64, warmup_steps=4000, lr=1.0)
    return m, opt


def _cuda(batch):
    return tuple(t.cuda() for t in batch)


def _update_agrees(flat_a, flat_b, p0, what):
    """The `0.05 lr0` rule on the elements whose (clamped, averaged) gradient is well above rounding noise: a first Adam update
    is lr * g / (|g| + eps), sign-like, so two runs are only comparable there."""
    from oracle import glow_oracle as O

    lr0 = O.noam_lr(1, 64, 4000)
    g = flat_b.flat_g
    big = g.abs() > 1e-3 * float(g.abs().max())
    assert bool(big.any())
    diff = ((flat_a.flat_p - p0) - (flat_b.flat_p - p0))[big].abs().max()
    assert float(diff) <= 0.05 * lr0, (what, float(diff), 0.05 * lr0)


# =============================================================================================== 1. the kernel
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "off1"])
@pytest.mark.parametrize("n", [1, 5, 1023, 4099, 2 ** 20 + 1])
def test_clip_grad_value_scaled_vs_torch(G, n, offset):
    clip = 0.25
    gen = torch.Generator(device="cuda").manual_seed(n + offset)
    base = 0.5 * torch.randn(n + 8, device="cuda", generator=gen)
    assert base.data_ptr() % 16 == 0
    for scale in (1.0, 0.5, 1.0 / 3.0):
        buf = base.clone()
        g = buf[offset: offset + n]
        assert (g.data_ptr() % 16 == 0) == (offset == 0)
        sumsq = torch.zeros(1, device="cuda")
        G.hip.call("glowtts_clip_grad_value_scaled", g.data_ptr(), n, scale, clip, sumsq.data_ptr())
        x = base[offset: offset + n] * torch.tensor(scale, device="cuda", dtype=torch.float32)
        want = x.clamp(-clip, clip)
        assert torch.equal(g, want), (n, offset, scale, float((g - want).abs().max()))
        # nothing outside [offset, offset + n) is written
        assert torch.equal(buf[:offset], base[:offset]) and torch.equal(buf[offset + n:], base[offset + n:])
        ref = float(x.double().pow(2).sum())
        print(f"clip_scaled n={n} offset={offset} scale={scale:.4f}: sumsq rel err {abs(float(sumsq) - ref) / ref:.2e}")
        assert abs(float(sumsq) - ref) <= 1e-5 * ref, (float(sumsq), ref)
        if n >= 1023:
            assert bool((x.abs() > clip).any()) and bool((x.abs() < clip).any())
        if scale == 1.0:                                   # bit for bit the unscaled kernel's result
            buf2 = base.clone()
            g2 = buf2[offset: offset + n]
            s2 = torch.zeros(1, device="cuda")
            G.hip.call("glowtts_clip_grad_value", g2.data_ptr(), n, clip, s2.data_ptr())
            assert torch.equal(g.view(torch.int32), g2.view(torch.int32))
            assert abs(float(sumsq) - float(s2)) <= 1e-5 * ref


def test_flat_adam_clip_takes_the_scale(G):
    clip = 0.25
    g0 = 0.5 * torch.randn(64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(9))
    flat = G.optimize.FlatAdam([torch.nn.Parameter(g0.clone())])
    flat.flat_g.copy_(g0)
    norm = flat.clip_grad_value_(clip, scale=0.5)
    assert torch.equal(flat.flat_g, (g0 * 0.5).clamp(-clip, clip))
    assert abs(float(norm) - float((g0 * 0.5).double().norm())) <= 1e-5 * float(norm)


# =============================================================================================== 2. every gradient accumulates
def test_every_gradient_accumulates(G, small, conv_mode):
    """Forward + backward of each micro-batch alone (from zero_grad, same weights, no update) against the three as one
    accumulation: the accumulated flat gradient is the sum of the three, per parameter tensor, within the project's gradient
    criterion.  A kernel that overwrites a gradient instead of adding to it fails here.

    Measured on an MI355X (profiles/r07_accum_bench.txt): worst |difference| / tolerance over all tensors 0.0001 in both
    arithmetics (decoder.flows.4.weight)."""
    model, opt = _model(G, small)
    flat = opt._optim
    batches = [_cuda(b) for b in small.batches]
    singles = []
    for b in batches:
        G.train._accumulate(model, opt, [b])
        singles.append(flat.flat_g.clone())
    want = singles[0] + singles[1] + singles[2]
    losses = G.train._accumulate(model, opt, batches)
    got = flat.flat_g.clone()
    assert len(losses) == 3 and opt.step_num == 1
    gmax = float(want.abs().max())
    names = [n for n, _ in model.named_parameters()]
    worst, worst_name = 0.0, None
    for name, (o, n) in zip(names, flat.slices()):
        w, g = want[o:o + n], got[o:o + n]
        tol = 5e-3 * float(w.abs().max()) + 1e-5 * gmax
        margin = float((g - w).abs().max()) / tol
        if margin > worst:
            worst, worst_name = margin, name
        # the sum is not any single contribution: a tensor whose gradient one micro-batch overwrote equals that micro-batch's
        assert float((g - w).abs().max()) <= tol, (name, margin)
    print(f"accumulation margin [{conv_mode}]: worst |accumulated - sum of singles| / tolerance = {worst:.4f} ({worst_name})")
    # the check has teeth: the last micro-batch's gradient alone is far outside the tolerance for most tensors
    outside = 0
    for o, n in flat.slices():
        w = want[o:o + n]
        outside += float((singles[2][o:o + n] - w).abs().max()) > 5e-3 * float(w.abs().max()) + 1e-5 * gmax
    assert outside > 0.5 * len(names), outside


# =============================================================================================== 3. one update vs the oracle
@pytest.fixture(scope="module")
def oracle_two(small):
    """The CPU oracle's update from the first two micro-batches: per-batch gradients averaged, clamped, one Adam/Noam step."""
    from oracle import glow_oracle as O

    hp = small.hp
    sdo = {k: v.clone().requires_grad_(True) for k, v in small.sd.items()}
    grads, losses = [], []
    for batch in small.batches[:2]:
        x, xl, y, yl, spk = batch
        for p in sdo.values():
            p.grad = None
        (z, z_m, z_logs, logdet, z_mask), _, (_attn, logw, logw_) = O.generator_forward(sdo, hp, x, xl, y, yl, spk)
        loss = O.mle_loss(z, z_m, z_logs, logdet, z_mask) + O.duration_loss(logw, logw_, xl)
        loss.backward()
        losses.append(float(loss.detach()))
        grads.append({k: p.grad.clone() for k, p in sdo.items() if p.grad is not None})
    mean = {k: (grads[0][k] + grads[1][k]) / 2 for k in grads[0]}
    assert set(grads[0]) == set(grads[1])
    O.clip_grad_value(mean.values(), CLIP)
    oopt = O.AdamNoam(dict(sdo), dim_model=64)
    oopt.step(mean)
    return types.SimpleNamespace(loss=sum(losses) / 2, grads=mean, params={k: v.detach() for k, v in sdo.items()})


def test_one_update_from_two_micro_batches_vs_oracle(G, small, oracle_two, conv_mode):
    from oracle import glow_oracle as O

    model, opt = _model(G, small)
    loss = G.train.train_batches(model, opt, [_cuda(b) for b in small.batches[:2]], CLIP)
    assert loss.is_cuda and loss.dim() == 0
    assert abs(float(loss) - oracle_two.loss) <= 1e-3 * abs(oracle_two.loss), (float(loss), oracle_two.loss)
    assert opt.step_num == 2
    assert float(opt._optim.dev_state[0]) == 2.0 and float(opt._optim.dev_state[1]) == 2.0
    named = dict(model.named_parameters())
    gmax = max(float(g.abs().max()) for g in oracle_two.grads.values())
    for k, g in oracle_two.grads.items():          # the averaged, clamped gradients, tensor by tensor
        assert_close(named[k].grad, g, what="grad " + k, rtol=0, atol=5e-3 * float(g.abs().max()) + 1e-5 * gmax)
    now = model.state_dict()
    lr0 = O.noam_lr(1, 64, 4000)
    for k, g in oracle_two.grads.items():
        big = g.abs() > 1e-3 * gmax
        if not bool(big.any()):
            continue
        upd_o = (oracle_two.params[k] - small.sd[k])[big]
        upd_h = (now[k].cpu() - small.sd[k])[big]
        assert float((upd_h - upd_o).abs().max()) <= 0.05 * lr0, k


# =============================================================================================== 4. packs once per update
def _count_weight_work(G, monkeypatch):
    """Count the launches that depend on the weights alone, wherever the package's modules call them from."""
    import glow_tts_train

    counts = {"n": 0}
    real = G.hip.call

    def counting(name, *args, **kw):
        if name.startswith(("glowtts_pack_weight", "glowtts_wino_weights", "glowtts_invconv_prepare")):
            counts["n"] += 1
        return real(name, *args, **kw)

    import importlib
    import pkgutil
    for info in pkgutil.iter_modules(glow_tts_train.__path__):
        mod = importlib.import_module("glow_tts_train." + info.name)
        if getattr(mod, "call", None) is real:
            monkeypatch.setattr(mod, "call", counting)

    def take():
        n, counts["n"] = counts["n"], 0
        return n

    return take


def test_weights_are_packed_once_per_update_and_never_stale(G, small, monkeypatch, conv_mode):
    batches = [_cuda(b) for b in small.batches]
    take = _count_weight_work(G, monkeypatch)
    ref_model, ref_opt = _model(G, small)
    take()
    G.train.train_batch(ref_model, ref_opt, batches[0], CLIP)
    plain = take()
    assert plain > 0

    model, opt = _model(G, small)
    p0 = opt._optim.flat_p.clone()
    take()
    G.train.train_batches(model, opt, batches, CLIP)
    first = take()
    p1 = opt._optim.flat_p.clone()
    assert not G.hip.weights_state.active and not G.hip.weights_state.record and not G.hip.weights_state.loose
    G.train.train_batches(model, opt, batches, CLIP)
    second = take()
    assert first == plain and second == plain, (plain, first, second)

    # the same update with every micro-batch packing for itself: more launches, the same parameters
    model2, opt2 = _model(G, small)
    take()
    G.train.train_batches(model2, opt2, batches, CLIP, reuse_packs=False)
    assert take() == 3 * plain
    holder = types.SimpleNamespace(flat_p=p1, flat_g=opt2._optim.flat_g)
    _update_agrees(holder, opt2._optim, p0, "reuse vs no reuse")

    # never stale: move the weights well beyond an update's size on both models (same values), then accumulate once more — with
    # reuse on one, without on the other.  Packs left over from the previous update would give the gradients of the old weights.
    opt2._optim.flat_p.copy_(opt._optim.flat_p)
    noise = 0.02 * torch.randn(opt._optim.flat_p.shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    opt._optim.flat_p.add_(noise)
    opt2._optim.flat_p.add_(noise)
    take()
    G.train._accumulate(model, opt, batches)
    assert take() == plain
    G.train._accumulate(model2, opt2, batches, reuse_packs=False)
    ga, gb = opt._optim.flat_g, opt2._optim.flat_g
    gmax = float(gb.abs().max())
    for name, (o, n) in zip([k for k, _ in model.named_parameters()], opt._optim.slices()):
        tol = 5e-3 * float(gb[o:o + n].abs().max()) + 1e-5 * gmax
        assert float((ga[o:o + n] - gb[o:o + n]).abs().max()) <= tol, name

    # outside train_batches nothing is reused: a plain step packs again
    take()
    G.train.train_batch(model, opt, batches[0], CLIP)
    assert take() == plain
    assert opt.step_num == 4                                     # two updates and one plain step


# =============================================================================================== 5. API edges
def test_single_micro_batch_is_train_batch(G, small, monkeypatch):
    batch = _cuda(small.batches[0])
    launches = []
    real = G.hip.call

    def logging_call(name, *args, **kw):
        launches.append(name)
        return real(name, *args, **kw)

    import glow_tts_train.convops as convops
    import glow_tts_train.ops as ops
    import glow_tts_train.optimize as optimize
    for mod in (convops, ops, optimize, G.utils, G.train):
        if getattr(mod, "call", None) is real:
            monkeypatch.setattr(mod, "call", logging_call)
    m1, o1 = _model(G, small)
    p0 = o1._optim.flat_p.clone()
    G.train.train_batch(m1, o1, batch, CLIP)
    plain, launches[:] = list(launches), []
    m2, o2 = _model(G, small)
    loss = G.train.train_batches(m2, o2, [batch], CLIP)
    assert sorted(launches) == sorted(plain)          # the same launches (two streams' host order may interleave differently)
    assert "glowtts_clip_grad_value_scaled" not in launches
    assert loss.dim() == 0
    assert (o1.step_num, o1.cur_lr) == (o2.step_num, o2.cur_lr) == (2, o2.cur_lr)
    _update_agrees(o1._optim, o2._optim, p0, "train_batches([b]) vs train_batch")


def test_arguments_and_tail_group(G, small):
    model, opt = _model(G, small)
    cfg = types.SimpleNamespace(grad_clip=CLIP)
    with pytest.raises(ValueError):
        G.train.train_batches(model, opt, [], CLIP)
    with pytest.raises(ValueError, match="accum_steps"):
        G.train.train_step(1, 1, model, opt, cfg, [], accum_steps=0)
    with pytest.raises(ValueError, match="GradScaler"):
        G.train.train_step(1, 1, model, opt, cfg, [], scaler=object(), accum_steps=2)
    assert opt.step_num == 1
    loader = [small.batches[2], small.batches[1], small.batches[2], small.batches[2], small.batches[1]]   # CPU batches
    seen = []
    step = G.train.train_step(7, 1, model, opt, cfg, loader, accum_steps=2, on_loss=lambda e, loss, s: seen.append((e, loss, s)))
    assert step == 10 and opt.step_num == 4                     # 2 + 2 + 1 batches: three updates
    assert float(opt._optim.dev_state[0]) == 4.0
    assert len(seen) == 1 and seen[0][0] == 1 and seen[0][2] == 10 and seen[0][1] == seen[0][1]     # (finite: not NaN)
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
