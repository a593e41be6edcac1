"""GPU tests (-m gpu) of `skip_nonfinite`: an update whose gradient holds a NaN or an Inf is skipped on the device.

Kernel level: glowtts_clip_grad_value_guarded against torch and against the unguarded kernels, glowtts_adam_noam_guarded +
glowtts_adam_advance_guarded against the unguarded pair.  Step level (the small model of tests/test_grad_accum.py): a poisoned
update is skipped and the run recovers, the same through train_batches, the per-tensor clip route, "off means off", the epoch's
plumbing in train_step, and two data-parallel ranks of which one is poisoned.

The loss is poisoned, never the inputs: train.mle_loss is patched to multiply its result by a device scalar (1, nan or inf), so
the backward carries non-finite values through arithmetic only and the alignment search always sees finite scores.

Bounds: everything a skipped update must leave alone, and everything a clean guarded update shares with the unguarded kernels,
is compared bit for bit.  sumsq: 1e-5 of the fp64 sum, the project's figure for this reduction (tests/test_grad_accum.py).  Two
whole steps of the model are not bit-repeatable (float atomics): a recovered run meets its twin inside `_close_to_twin`'s bound."""
import logging
import os
import socket
import types

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CLIP = 5.0
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def G():
    from glow_tts_train import _hip, convops, models, optimize, train, utils

    _hip.load()
    return types.SimpleNamespace(hip=_hip, convops=convops, models=models, optimize=optimize, train=train, utils=utils)


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# =============================================================================================== 1. the guarded clip kernel
# 1, 5, 1023, 4099, 2^20 + 1: the scalar form (n % 4 != 0) up to more than one grid-stride pass (512 workgroups x 256 threads x 4
# loads = 524288 elements per pass); 4100 and 2^21 + 4: the same for the vector form (one float4 per load), which needs n % 4 == 0
# and an aligned pointer — with offset 1 they take the scalar form over the same data.
CLIP_N = [1, 5, 1023, 4099, 4100, 2 ** 20 + 1, 2 ** 21 + 4]
KCLIP = 0.25


@pytest.fixture(scope="module")
def clip_base():
    """One random buffer per n (0.5 N(0, 1): values on both sides of the clamp), made once and never written."""
    out = {}
    for n in CLIP_N:
        gen = torch.Generator(device="cuda").manual_seed(n)
        out[n] = 0.5 * torch.randn(n + 8, device="cuda", generator=gen)
        assert out[n].data_ptr() % 16 == 0
    return out


def _guarded_clip(G, g, n, scale, guard, clip=KCLIP):
    sumsq = torch.zeros(1, device="cuda")
    G.hip.call("glowtts_clip_grad_value_guarded", g.data_ptr(), n, scale, clip, sumsq.data_ptr(), guard.data_ptr())
    return sumsq


def _fresh_guard(flag=0.0):
    return torch.tensor([flag, 7.0, 8.0, 9.0], device="cuda")            # the counters are not the clip pass's to touch


@pytest.mark.parametrize("scale", [1.0, 0.25])
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "off1"])
@pytest.mark.parametrize("n", CLIP_N)
def test_guarded_clip_clean_input(G, clip_base, n, offset, scale):
    base = clip_base[n]
    buf = base.clone()
    g = buf[offset: offset + n]
    assert (g.data_ptr() % 16 == 0) == (offset == 0)
    guard = _fresh_guard()
    sumsq = _guarded_clip(G, g, n, scale, guard)
    # bit for bit the unguarded kernel of the same scale
    buf2 = base.clone()
    g2 = buf2[offset: offset + n]
    s2 = torch.zeros(1, device="cuda")
    if scale == 1.0:
        G.hip.call("glowtts_clip_grad_value", g2.data_ptr(), n, KCLIP, s2.data_ptr())
    else:
        G.hip.call("glowtts_clip_grad_value_scaled", g2.data_ptr(), n, scale, KCLIP, s2.data_ptr())
    assert _bits_equal(buf, buf2)                                           # (the whole buffer: nothing outside [offset, offset + n))
    x = base[offset: offset + n] * torch.tensor(scale, device="cuda", dtype=torch.float32)
    assert torch.equal(g, x.clamp(-KCLIP, KCLIP))
    ref = float(x.double().pow(2).sum())
    print(f"clip_guarded n={n} offset={offset} scale={scale}: sumsq rel err {abs(float(sumsq) - ref) / ref:.2e} (bound 1e-5)")
    assert abs(float(sumsq) - ref) <= 1e-5 * ref, (float(sumsq), ref)
    assert guard.tolist() == [0.0, 7.0, 8.0, 9.0]
    # (d) a flag that is already set stays set after a clean pass (the per-tensor route accumulates into it)
    guard = _fresh_guard(1.0)
    _guarded_clip(G, base.clone()[offset: offset + n], n, scale, guard)
    assert guard.tolist() == [1.0, 7.0, 8.0, 9.0]


@pytest.mark.parametrize("scale", [1.0, 0.25])
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "off1"])
@pytest.mark.parametrize("n", CLIP_N)
def test_guarded_clip_flags_one_bad_element(G, clip_base, n, offset, scale):
    """NaN, +Inf, -Inf at the first index, the last index and inside the trailing partial block of 1024 elements (256 threads x 4)."""
    base = clip_base[n]
    where = sorted({0, n - 1, (n // 1024) * 1024 + (n % 1024) // 2})
    for idx in where:
        for bad in (NAN, INF, -INF):
            buf = base.clone()
            g = buf[offset: offset + n]
            g[idx] = bad
            guard = _fresh_guard()
            _guarded_clip(G, g, n, scale, guard)
            got = guard.tolist()
            assert got[0] != 0.0 and got[1:] == [7.0, 8.0, 9.0], (n, offset, scale, idx, bad, got)
            # what the issue is about: after the clamp the bad element is an ordinary finite number
            assert bool(torch.isfinite(g).all())


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "off1"])
@pytest.mark.parametrize("n", [5, 4100])
def test_guarded_clip_flag_is_per_element_not_per_sum(G, clip_base, n, offset):
    """3e38 * 0.25 is finite, its square is not: sumsq overflows to Inf and the flag stays clear.  The test is on x = g * scale, so
    the same element with scale 4 (x = Inf) does set it."""
    for scale in (0.25, 4.0):
        buf = clip_base[n].clone()
        g = buf[offset: offset + n]
        g[n // 2] = 3e38
        guard = _fresh_guard()
        sumsq = _guarded_clip(G, g, n, scale, guard)
        assert float(sumsq) == INF
        if scale == 0.25:
            assert guard.tolist() == [0.0, 7.0, 8.0, 9.0]
        else:
            assert guard[0] != 0.0 and guard.tolist()[1:] == [7.0, 8.0, 9.0]


# =============================================================================================== 2. guarded Adam + advance
HYPER = (0.01, 0.9, 0.98, 1e-9, 192.0, 4000.0)                               # lr, b1, b2, eps, dim_model, warmup
STATE0 = [4.0, 2.0, 123.0, 0.0241]                                           # t != step_num, a pending imposed rate


def _adam_buffers(n):
    gen = torch.Generator(device="cuda").manual_seed(n)
    p = torch.randn(n, device="cuda", generator=gen)
    g = torch.randn(n, device="cuda", generator=gen)
    m = 0.1 * torch.randn(n, device="cuda", generator=gen)
    v = 0.1 * torch.rand(n, device="cuda", generator=gen)
    return p, g, m, v


def _guarded_update(G, p, g, m, v, state, guard):
    lr, b1, b2, eps, dim, warm = HYPER
    G.hip.call("glowtts_adam_noam_guarded", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), state.data_ptr(),
               guard.data_ptr(), lr, b1, b2, eps, dim, warm)
    G.hip.call("glowtts_adam_advance_guarded", state.data_ptr(), guard.data_ptr(), lr, dim, warm)


def _plain_update(G, p, g, m, v, state):
    lr, b1, b2, eps, dim, warm = HYPER
    G.hip.call("glowtts_adam_noam", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), state.data_ptr(),
               lr, b1, b2, eps, dim, warm)
    G.hip.call("glowtts_adam_advance", state.data_ptr(), lr, dim, warm)


@pytest.mark.parametrize("n", [64, 4100])
def test_guarded_adam_and_advance(G, n):
    p0, g0, m0, v0 = _adam_buffers(n)
    st0 = torch.tensor(STATE0, device="cuda")
    # ---- the unguarded pair
    pu, mu, vu, su = p0.clone(), m0.clone(), v0.clone(), st0.clone()
    _plain_update(G, pu, g0, mu, vu, su)
    assert not _bits_equal(pu, p0) and su.tolist()[:2] == [5.0, 3.0] and float(su[3]) == 0.0
    # ---- clean: bit for bit the unguarded pair
    p, m, v, st, guard = p0.clone(), m0.clone(), v0.clone(), st0.clone(), torch.zeros(4, device="cuda")
    _guarded_update(G, p, g0, m, v, st, guard)
    assert _bits_equal(p, pu) and _bits_equal(m, mu) and _bits_equal(v, vu) and _bits_equal(st, su)
    assert guard.tolist() == [0.0, 0.0, 0.0, 1.0]
    # ---- bad: nothing moves, the imposed rate is not used up
    p, m, v, st = p0.clone(), m0.clone(), v0.clone(), st0.clone()
    guard = torch.tensor([1.0, 0.0, 0.0, 0.0], device="cuda")
    g_bad = torch.full_like(g0, NAN)
    _guarded_update(G, p, g_bad, m, v, st, guard)
    assert _bits_equal(p, p0) and _bits_equal(m, m0) and _bits_equal(v, v0) and _bits_equal(st, st0)
    assert guard.tolist() == [0.0, 1.0, 1.0, 0.0]
    # ---- bad, bad, clean: the state has advanced exactly once
    guard[0] = 1.0
    _guarded_update(G, p, g_bad, m, v, st, guard)
    assert guard.tolist() == [0.0, 2.0, 2.0, 0.0] and _bits_equal(st, st0) and _bits_equal(p, p0)
    _guarded_update(G, p, g0, m, v, st, guard)
    assert guard.tolist() == [0.0, 2.0, 0.0, 1.0]
    assert _bits_equal(p, pu) and _bits_equal(m, mu) and _bits_equal(v, vu) and _bits_equal(st, su)


# =============================================================================================== the small model
# (b, t_text, t_mel, text lengths, mel lengths, speakers)
BATCHES = [
    (2, 12, 64, [12, 7], [64, 33], [1, 2]),
    (2, 10, 56, [10, 6], [56, 40], [0, 3]),
    (2, 12, 48, [12, 9], [48, 31], [2, 0]),
    (2, 8, 64, [8, 5], [64, 50], [3, 1]),
]


@pytest.fixture(scope="module")
def small():
    """The small multi-speaker config of tests/test_grad_accum.py (hidden 64, 3 blocks, 2 WN layers, dropout 0), B = 2, T_mel <= 64."""
    from oracle import glow_oracle as O

    hp = O.HParams(n_vocab=60, hidden_channels=64, filter_channels=128, filter_channels_dp=64, n_layers_enc=2,
                   n_blocks_dec=3, n_block_layers=2, n_speakers=4, gin_channels=16, mean_only=False)
    sd = O.init_state_dict(hp, seed=5)
    gen = torch.Generator().manual_seed(1)
    for k in list(sd):
        if k.endswith(".end.weight"):
            sd[k] = 0.05 * torch.randn(sd[k].shape, generator=gen)
    batches = []
    for b, tx, ty, xl, yl, spk in BATCHES:
        xl, yl = torch.tensor(xl), torch.tensor(yl)
        x = torch.randint(1, 60, (b, tx), generator=gen) * (torch.arange(tx)[None] < xl[:, None])
        y = torch.randn(b, 80, ty, generator=gen) * (torch.arange(ty)[None, None] < yl[:, None, None])
        batches.append((x, xl, y, yl, torch.tensor(spk)))
    return types.SimpleNamespace(hp=hp, sd=sd, batches=batches)


def _model(G, small, skip):
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
    opt = G.optimize.Adam(m.parameters(), scheduler="noam", dim_model=64, warmup_steps=4000, lr=1.0, skip_nonfinite=skip)
    return m, opt


def _cuda(batch):
    return tuple(t.cuda() for t in batch)


@pytest.fixture
def fp32_math(G):
    """fp32 conv math: this model's weight gradients then carry no float-atomic split."""
    before = G.convops.set_conv_math("fp32")
    yield
    G.convops.set_conv_math(before)


@pytest.fixture
def poison(G, monkeypatch):
    """train.mle_loss times a device scalar per call: `poison.plan(1, NAN)` sets the factors of the next calls, 1 afterwards.  Every
    call multiplies (by a device 1 when clean), so poisoned and clean runs launch the same kernels."""
    real = G.train.mle_loss
    state = types.SimpleNamespace(queue=[], one=torch.ones((), device="cuda"))

    def poisoned(*args):
        factor = state.queue.pop(0) if state.queue else state.one
        return real(*args) * factor

    monkeypatch.setattr(G.train, "mle_loss", poisoned)
    state.plan = lambda *values: state.queue.__setitem__(slice(None), [torch.tensor(float(v), device="cuda") for v in values])
    return state


def _snapshot(flat):
    return [t.clone() for t in (flat.flat_p, flat.flat_m, flat.flat_v, flat.dev_state)]


def _same(flat, snap):
    return all(_bits_equal(a, b) for a, b in zip((flat.flat_p, flat.flat_m, flat.flat_v, flat.dev_state), snap))


# =============================================================================================== 4. skipped, and the run recovers
def _close_to_twin(flat, twin, what):
    """`flat` against `twin` after the same clean updates.  Two runs of this step are not bit-repeatable (float atomics in the flows'
    and norms' reductions add in another order), so: device state bit for bit (no atomic feeds it); moments within what a gradient
    error of e_g = 2 ulp of max|g| (2^-22 max|g|, one rounding per order of summation and side) can leave after two updates from
    zero moments — m: (1 - b1)(1 + b1) e_g, v: (1 - b2)(1 + b2) 2 max|g| e_g; parameters by the project's `0.05 lr0` rule on the
    elements whose gradient is well above that noise (tests/test_grad_accum.py).  Returns the three figures."""
    from oracle import glow_oracle as O

    assert _bits_equal(flat.dev_state, twin.dev_state), what
    b1, b2 = twin.param_groups[0]["betas"]
    gmax = float(twin.flat_g.abs().max())
    e_g = 2.0 ** -22 * gmax
    dm = float((flat.flat_m - twin.flat_m).abs().max())
    dv = float((flat.flat_v - twin.flat_v).abs().max())
    big = twin.flat_g.abs() > 1e-3 * gmax
    dp = float((flat.flat_p - twin.flat_p)[big].abs().max())
    bm, bv, bp = (1 - b1) * (1 + b1) * e_g, (1 - b2) * (1 + b2) * 2 * gmax * e_g, 0.05 * O.noam_lr(1, 64, 4000)
    print(f"{what}: max|dm| {dm:.3e} (bound {bm:.3e}), max|dv| {dv:.3e} (bound {bv:.3e}), max|dp| on large-gradient elements {dp:.3e} "
          f"(bound {bp:.3e}), {int((flat.flat_p.view(torch.int32) != twin.flat_p.view(torch.int32)).sum())} parameters differ in bits")
    assert dm <= bm and dv <= bv and dp <= bp, (what, dm, bm, dv, bv, dp, bp)
    return dm, dv, dp


@pytest.mark.parametrize("bad", [NAN, INF], ids=["nan", "inf"])
def test_a_poisoned_update_is_skipped_and_the_run_recovers(G, small, poison, fp32_math, bad):
    """Clean, poisoned, clean on one batch.  After the poisoned step parameters, moments and device state are bit-equal to their
    values after the first — no tolerance there.  After the third they agree with an UNGUARDED twin that ran only the two clean steps.

    That last comparison cannot be bit for bit: two unguarded runs of the two clean steps already differ (measured on an MI355X, fp32
    conv math, five pairs, profiles/r08_guard_bench.txt: 300-500 clamped gradient elements by up to 4.7e-8 at max|g| 2.59, m by up
    to 6.3e-9, v by up to 1.5e-10, parameters identical).  A second unguarded twin runs first and is held to the same bound as
    the recovered run (_close_to_twin: moments within what 2 ulp of max|g| of gradient error leaves — 1.2e-7 for m, 1.3e-7 for v
    here — parameters by the `0.05 lr0` rule).  A poisoned update that was applied moves m by about (1 - b1) clip = 0.5 and every
    parameter by a learning rate."""
    batch = _cuda(small.batches[0])
    twin_m, twin = _model(G, small, skip=False)
    twin2_m, twin2 = _model(G, small, skip=False)
    for _ in range(2):
        G.train.train_batch(twin_m, twin, batch, CLIP)
        G.train.train_batch(twin2_m, twin2, batch, CLIP)
    _close_to_twin(twin2._optim, twin._optim, "two unguarded runs of two clean steps")

    model, opt = _model(G, small, skip=True)
    flat = opt._optim
    p0 = flat.flat_p.clone()
    loss1 = G.train.train_batch(model, opt, batch, CLIP)
    after_first = _snapshot(flat)
    assert not _bits_equal(flat.flat_p, p0)
    poison.plan(bad)
    loss2 = G.train.train_batch(model, opt, batch, CLIP)
    assert not bool(torch.isfinite(loss2)) and bool(torch.isfinite(loss1))
    assert _same(flat, after_first)
    assert flat.guard.tolist() == [0.0, 1.0, 1.0, 1.0]
    assert opt.step_num == 3                                                 # the mirror counted the attempt ...
    G.train.train_batch(model, opt, batch, CLIP)
    _close_to_twin(flat, twin._optim, "clean, poisoned, clean against two clean steps")
    counts = opt.sync_from_device()                                          # ... and is reconciled here
    assert counts == {"applied": 2, "skipped": 1, "consecutive_skipped": 0}
    assert (opt.step_num, opt.cur_lr) == (twin.step_num, twin.cur_lr) == (3, twin.cur_lr)
    assert opt._optim.param_groups[0]["lr"] == twin._optim.param_groups[0]["lr"]
    assert bool(torch.isfinite(flat.flat_p).all())


# =============================================================================================== 5. through train_batches
def test_a_poisoned_micro_batch_skips_the_whole_update(G, small, poison, fp32_math, monkeypatch):
    model, opt = _model(G, small, skip=True)
    flat = opt._optim
    batches = [_cuda(b) for b in small.batches[:2]]
    clips = []
    real = G.hip.call

    def recording(name, *args, **kw):
        if "clip_grad_value" in name:
            clips.append((name, args[2]))
        return real(name, *args, **kw)

    monkeypatch.setattr(G.optimize, "call", recording)
    before = _snapshot(flat)
    poison.plan(1, NAN)
    loss = G.train.train_batches(model, opt, batches, CLIP)
    assert clips == [("glowtts_clip_grad_value_guarded", 0.5)]
    assert not bool(torch.isfinite(loss))
    assert _same(flat, before)
    assert flat.guard.tolist() == [0.0, 1.0, 1.0, 0.0]
    G.train.train_batches(model, opt, batches, CLIP)                         # and the next update is applied
    assert not _bits_equal(flat.flat_p, before[0]) and bool(torch.isfinite(flat.flat_p).all())
    assert opt.sync_from_device() == {"applied": 1, "skipped": 1, "consecutive_skipped": 0} and opt.step_num == 2


# =============================================================================================== 6. the per-tensor route
def test_per_tensor_clip_route_sets_the_flag(G, small):
    """One parameter's .grad replaced by a foreign tensor holding an Inf: utils.clip_grad_value_, as train_batch calls it and as
    train_batches does for an accumulated gradient (scale=0.5), clamps tensor by tensor, every launch accumulating into the owner's
    flag; the update is skipped."""
    model, opt = _model(G, small, skip=True)
    flat = opt._optim
    params = list(model.parameters())
    for route in ("utils", "train"):
        opt.zero_grad()
        flat.flat_g.fill_(0.5)
        victim = params[0]                                                   # the FIRST launch sets the flag, all later ones are clean
        foreign = torch.full_like(victim, 9.0)
        foreign.view(-1)[1] = INF
        victim.grad = foreign
        assert flat.clip_grad_value_(CLIP) is None
        before = _snapshot(flat)
        if route == "utils":
            G.utils.clip_grad_value_(model.parameters(), CLIP)
            assert float(victim.grad.max()) == CLIP
        else:
            G.utils.clip_grad_value_(model.parameters(), CLIP, scale=0.5)
            assert float(victim.grad.max()) == CLIP and float(victim.grad.min()) == 4.5
        assert float(flat.guard[0]) != 0.0
        opt.step()
        assert _same(flat, before) and flat.grads_in_place()
    assert opt.sync_from_device() == {"applied": 0, "skipped": 2, "consecutive_skipped": 2} and opt.step_num == 1
    # a clean gradient on the same route is applied
    opt.zero_grad()
    flat.flat_g.fill_(0.5)
    params[0].grad = torch.full_like(params[0], 9.0)
    G.utils.clip_grad_value_(model.parameters(), CLIP)
    opt.step()
    assert flat.guard.tolist() == [0.0, 2.0, 0.0, 1.0] and not _bits_equal(flat.flat_p, before[0])


# =============================================================================================== 7. off means off
def _record_calls(G, monkeypatch):
    import glow_tts_train.convops as convops
    import glow_tts_train.ops as ops

    launches = []
    real = G.hip.call

    def logging_call(name, *args, **kw):
        launches.append(name)
        return real(name, *args, **kw)

    for mod in (convops, ops, G.optimize, G.utils, G.train):
        if getattr(mod, "call", None) is real:
            monkeypatch.setattr(mod, "call", logging_call)
    return launches


def test_off_means_off(G, small, monkeypatch):
    """Without the option no `_guarded` entry point is called and the step ends in clip, adam_noam, adam_advance as it always has;
    with it the launches are the same ones with those three replaced by their guarded forms."""
    launches = _record_calls(G, monkeypatch)
    batches = [_cuda(b) for b in small.batches[:2]]
    tail = ["glowtts_clip_grad_value", "glowtts_adam_noam", "glowtts_adam_advance"]
    runs = {}
    for skip in (False, True):
        model, opt = _model(G, small, skip=skip)
        launches.clear()
        G.train.train_batch(model, opt, batches[0], CLIP)
        one = list(launches)
        launches.clear()
        G.train.train_batches(model, opt, batches, CLIP)
        runs[skip] = (one, list(launches))
    one, two = runs[False]
    assert not [n for n in one + two if n.endswith("_guarded")]
    assert one[-3:] == tail and two[-3:] == ["glowtts_clip_grad_value_scaled"] + tail[1:]
    assert sum(n in tail or n == "glowtts_clip_grad_value_scaled" for n in one) == 3
    assert sum(n in tail or n == "glowtts_clip_grad_value_scaled" for n in two) == 3
    guarded = {"glowtts_clip_grad_value": "glowtts_clip_grad_value_guarded", "glowtts_adam_noam": "glowtts_adam_noam_guarded",
               "glowtts_clip_grad_value_scaled": "glowtts_clip_grad_value_guarded", "glowtts_adam_advance": "glowtts_adam_advance_guarded"}
    for off, on in zip(runs[False], runs[True]):
        assert sorted(guarded.get(n, n) for n in off) == sorted(on)          # (two streams' host order may interleave differently)
        assert on[-3:] == [guarded[n] for n in off[-3:]]


# =============================================================================================== 8. the epoch's plumbing
def test_train_step_reports_skips_at_the_epochs_sync_point(G, small, poison, monkeypatch, caplog):
    model, opt = _model(G, small, skip=True)
    cfg = types.SimpleNamespace(grad_clip=CLIP)
    loader = list(small.batches)                                             # four CPU batches
    losses = []
    real_batch = G.train.train_batch

    def recording(*args, **kw):
        losses.append(real_batch(*args, **kw))
        return losses[-1]

    monkeypatch.setattr(G.train, "train_batch", recording)
    seen = []
    poison.plan(1, NAN, 1, 1)
    with caplog.at_level(logging.WARNING, logger="glow_tts_train"):
        step = G.train.train_step(7, 1, model, opt, cfg, loader, skip_nonfinite=True, on_loss=lambda e, loss, s: seen.append((e, loss, s)))
    assert step == 11                                                        # update attempts, as without the option
    host = [float(t) for t in losses]
    assert len(host) == 4 and host[1] != host[1] and all(h == h for h in host[:1] + host[2:])
    want = float(np.mean(np.array(host[:1] + host[2:], dtype=np.float32).astype(np.float64)))
    assert len(seen) == 1 and seen[0][0] == 1 and seen[0][2] == 11
    assert seen[0][1] == pytest.approx(want, rel=1e-6)                       # the mean over the three finite losses (fp32 on device)
    warnings = [r for r in caplog.records if r.levelno == logging.WARNING and r.name == "glow_tts_train"]
    assert len(warnings) == 1 and "1 of 4" in warnings[0].getMessage()
    assert opt.step_num == 4 and opt._optim.guard.tolist() == [0.0, 1.0, 0.0, 3.0]

    # every update of an epoch skipped: that run is not training
    before = _snapshot(opt._optim)
    poison.plan(NAN, INF, NAN, -INF)
    with pytest.raises(RuntimeError, match="skipped"):
        G.train.train_step(11, 2, model, opt, cfg, loader, skip_nonfinite=True)
    assert _same(opt._optim, before) and opt.step_num == 4

    # refusals
    with pytest.raises(ValueError, match="GradScaler"):
        G.train.train_step(1, 1, model, opt, cfg, loader, fp16_run=True, scaler=object())
    with pytest.raises(ValueError, match="GradScaler"):
        G.train.train_batch(model, opt, _cuda(loader[0]), CLIP, scaler=object())
    plain_model, plain = _model(G, small, skip=False)
    with pytest.raises(ValueError, match="skip_nonfinite=True"):
        G.train.train_step(1, 1, plain_model, plain, cfg, loader, skip_nonfinite=True)
    assert _same(opt._optim, before)


# =============================================================================================== 9. two ranks, one poisoned
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_worker(rank, world, port, q):
    import sys
    import torch.distributed as dist

    sys.path[:0] = [os.path.join(ROOT, "glow-tts-train_amd"), ROOT]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    from glow_tts_train import models, optimize, parallel, train

    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.manual_seed(1234)
        model = models.FlowGenerator(n_vocab=60, hidden_channels=64, filter_channels=128, filter_channels_dp=64, out_channels=80,
                                     kernel_size=3, n_heads=2, n_layers_enc=2, p_dropout=0.0, n_blocks_dec=3, kernel_size_dec=5,
                                     dilation_rate=1, n_block_layers=2, p_dropout_dec=0.0, n_split=4, n_sqz=2, window_size=4,
                                     mean_only=True, prenet=True).cuda().train()
        for m in model.modules():
            if isinstance(m, torch.nn.Dropout):
                m.p = 0.0
        with torch.no_grad():
            for f in model.decoder.flows:
                if hasattr(f, "end"):
                    f.end.weight.normal_(0, 0.01)
        opt = optimize.Adam(model.parameters(), scheduler="noam", dim_model=64, warmup_steps=4000, lr=1.0, skip_nonfinite=True)
        red = parallel.FlowBlockReducer(model, opt)
        red.broadcast_parameters(0)
        gen = torch.Generator().manual_seed(500 + rank)
        xl, yl = torch.tensor([12, 7]), torch.tensor([64, 33])
        x = torch.randint(1, 60, (2, 12), generator=gen) * (torch.arange(12)[None] < xl[:, None])
        y = torch.randn(2, 80, 64, generator=gen) * (torch.arange(64)[None, None] < yl[:, None, None])
        batch = (x.cuda(), xl.cuda(), y.cuda(), yl.cuda(), None)
        factor = torch.tensor(NAN if rank == 1 else 1.0, device="cuda")      # only rank 1's loss is poisoned
        real = train.mle_loss
        train.mle_loss = lambda *a: real(*a) * factor
        before = opt._optim.flat_p.detach().cpu().numpy().copy()
        loss = train.train_batch(model, opt, batch, 5.0, red)
        counts = opt.sync_from_device()
        after = opt._optim.flat_p.detach().cpu().numpy().copy()
        q.put((rank, counts, bool(torch.isfinite(loss)), before, after, opt.step_num))
    finally:
        dist.destroy_process_group()


def test_two_ranks_skip_together_when_one_is_poisoned():
    """gloo, both ranks on the one card, FlowBlockReducer: the all-reduce carries rank 1's NaN into both ranks' flat gradient, the
    element test is independent of order, so both skip — bit-equal parameters before and after, on both ranks."""
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=180) for _ in range(world)), key=lambda r: r[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    (_, c0, finite0, before0, after0, s0), (_, c1, finite1, before1, after1, s1) = res
    assert finite0 and not finite1                                           # rank 0's own loss was fine
    assert c0 == c1 == {"applied": 0, "skipped": 1, "consecutive_skipped": 1}
    assert s0 == s1 == 1
    assert np.array_equal(before0.view(np.int32), after0.view(np.int32))
    assert np.array_equal(before1.view(np.int32), after1.view(np.int32))
    assert np.array_equal(after0.view(np.int32), after1.view(np.int32))
