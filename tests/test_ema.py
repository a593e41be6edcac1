"""GPU tests (-m gpu) of the exponential moving average of the weights that the update kernel keeps (`ema_decay`).

Kernel level: glowtts_adam_noam_ema against glowtts_adam_noam (p, m, v bit for bit) and against fp64 (e), its guard, and
glowtts_swap_f32.  Optimizer and step level (the small model of tests/test_grad_accum.py): the average follows the fp64 recurrence
over three updates, "off means off", a skipped update leaves it alone, `swap_ema()`, the checkpoints `train()` writes, and two
data-parallel ranks.

Bounds.  Everything that is moved, left alone or shared with the plain kernel: bit for bit.  The average itself, per element:
|e_new - (e + a (p' - e))| <= 16 u (|e| + |p'|), u = 2**-24, p' the device's own updated parameter and a the weight as the kernel
rounds it — 4 x the 2.37 u that the kernel's sequence of three fp32 operations shows against fp64 in numpy on the CPU on the same
inputs, rounded up to a power of two (tests/ema_cases.py; tests/test_ema_cpu.py re-measures it).  Over K updates the per-update
bounds add up (an earlier error is carried on with a factor 1 - a < 1)."""
import os
import socket
import types

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import ema_cases as C

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CLIP = 5.0
SENTINEL = -1234.5
NAN = float("nan")


@pytest.fixture(scope="module")
def G():
    from glow_tts_train import _hip, checkpoint, convops, models, optimize, train, utils

    _hip.load()
    return types.SimpleNamespace(hip=_hip, checkpoint=checkpoint, convops=convops, models=models, optimize=optimize, train=train,
                                 utils=utils)


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# =============================================================================================== 1. the raw kernel, guard = NULL
def _ema_call(G, bufs, offset, n, state, guard, case, t=C.STATE[0]):
    rate, warm, k = case
    p, g, m, v, e = (b[offset: offset + n] for b in bufs)
    G.hip.call("glowtts_adam_noam_ema", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), e.data_ptr(), n, state.data_ptr(),
               None if guard is None else guard.data_ptr(), C.LR, C.B1, C.B2, C.EPS, C.DIM, C.WARMUP, rate, warm, t - k)


@pytest.fixture(scope="module")
def adam_base():
    """(p, g, m, v, e) on the device per n, made once and never written; the tests work on clones."""
    out = {}
    for n in C.SIZES:
        out[n] = [t.cuda() for t in C.adam_ema_data(n)[:5]]
        assert all(t.data_ptr() % 16 == 0 for t in out[n])
    return out


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "off1"])
@pytest.mark.parametrize("n", C.SIZES)
def test_ema_update_raw(G, adam_base, n, offset):
    """glowtts_adam_noam_ema, guard = NULL, on buffers the test fills itself (n + 8 floats each, the kernel works on [offset, offset + n):
    what lies outside is the sentinel region).  p, m, v bit-equal to glowtts_adam_noam on clones; g, state and everything outside
    the range untouched; e against fp64 e + a (p' - e) with p' the device's own result, for a = 1e-4, a = 0.1 and the warm-up at
    k = 0, 5, 1e5 (a = 0.9, 0.6, 8.9991e-5) — bound 16 u (|e| + |p'|), see the module docstring; padding elements stay exactly 0."""
    base = adam_base[n]
    pad = C.adam_ema_data(n)[6][offset: offset + n].cuda()
    st0 = torch.tensor(C.STATE, dtype=torch.float32)
    # ---- the plain kernel on clones
    plain = [t.clone() for t in base[:4]]
    st = st0.cuda()
    G.hip.call("glowtts_adam_noam", *(t[offset: offset + n].data_ptr() for t in plain), n, st.data_ptr(), C.LR, C.B1, C.B2, C.EPS,
               C.DIM, C.WARMUP)
    assert not _bits_equal(plain[0], base[0])
    e64 = base[4][offset: offset + n].cpu()
    worst = 0.0
    for case in C.EMA_CASES:
        bufs = [t.clone() for t in base]
        assert (bufs[0][offset:].data_ptr() % 16 == 0) == (offset == 0)
        st = st0.cuda()
        _ema_call(G, bufs, offset, n, st, None, case)
        for got, want in zip(bufs[:4], plain):                             # p, g, m, v: the WHOLE buffers, so nothing outside the range
            assert _bits_equal(got, want), case
        assert _bits_equal(bufs[1], base[1]) and torch.equal(st.cpu(), st0)
        e = bufs[4]
        assert _bits_equal(e[:offset], base[4][:offset]) and _bits_equal(e[offset + n:], base[4][offset + n:])
        p_new = bufs[0][offset: offset + n].cpu()
        a = C.ema_weight(*case)
        fig = C.units(e[offset: offset + n], C.ema_ref(e64, p_new, a), e64.double().abs() + p_new.double().abs())
        print(f"ema n={n} offset={offset} rate={case[0]:g} warm={case[1]} k={case[2]}: a = {a:.7g}, e {fig:.2f} u (bound {C.E_BOUND:g})")
        worst = max(worst, fig)
        assert fig <= C.E_BOUND, (case, fig)
        assert bool((e[offset: offset + n][pad] == 0).all()) and bool((bufs[0][offset: offset + n][pad] == 0).all())
        if n >= 1023:
            assert not _bits_equal(e, base[4])
    if n >= 5:
        assert bool(pad.any()) and not bool(pad.all())
    print(f"ema n={n} offset={offset}: worst e {worst:.2f} u of |e| + |p'| (bound {C.E_BOUND:g})")


# =============================================================================================== 2. guarded
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "off1"])
@pytest.mark.parametrize("n", [5, 4099, 2 ** 21 + 4])
def test_ema_update_guarded(G, adam_base, n, offset):
    """Flag 0: p, m, v, e bit-equal to the guard = NULL call.  Flag 1: all four untouched bit for bit.  The guard is not written."""
    base = adam_base[n]
    case = C.EMA_CASES[3]
    st0 = torch.tensor(C.STATE, dtype=torch.float32)
    free = [t.clone() for t in base]
    _ema_call(G, free, offset, n, st0.cuda(), None, case)
    assert not _bits_equal(free[0], base[0]) and not _bits_equal(free[4], base[4])
    for flag in (0.0, 1.0, -3.0, NAN):
        bufs = [t.clone() for t in base]
        guard = torch.tensor([flag, 7.0, 8.0, 9.0], device="cuda")
        before = guard.clone()
        st = st0.cuda()
        _ema_call(G, bufs, offset, n, st, guard, case)
        want = free if flag == 0.0 else base
        assert all(_bits_equal(a, b) for a, b in zip(bufs, want)), flag
        assert _bits_equal(guard, before) and torch.equal(st.cpu(), st0)


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "off1"])
@pytest.mark.parametrize("n", [5, 4100])
def test_ema_guard_form_is_chosen_on_the_host(G, n, offset):
    """glowtts_adam_noam_ema instantiates the update kernel with or without the guard test from `guard != NULL` alone.  n = 5 takes the
    scalar form, n = 4100 the 16-byte one, and offset 1 forces the scalar form on it too.  Buffers of n + 8 floats, the kernel works
    on [offset, offset + n), and every comparison is over the WHOLE buffers, the eight floats around the range included.  guard NULL
    against a cleared guard: p, m, v, e bit-equal, and p, m, v bit-equal to glowtts_adam_noam on clones.  guard[0] = 1: p, m, v, e
    bit-unchanged.  The kernel never writes the guard."""
    base = [t.cuda() for t in C.adam_ema_data(n)[:5]]
    assert all(t.numel() == n + C.PAD and t.data_ptr() % 16 == 0 for t in base)
    case = C.EMA_CASES[3]
    st0 = torch.tensor(C.STATE, dtype=torch.float32)
    free = [t.clone() for t in base]
    _ema_call(G, free, offset, n, st0.cuda(), None, case)
    assert not _bits_equal(free[0], base[0]) and not _bits_equal(free[4], base[4])
    held = [t.clone() for t in base]
    guard = torch.zeros(4, device="cuda")
    _ema_call(G, held, offset, n, st0.cuda(), guard, case)
    plain = [t.clone() for t in base[:4]]
    G.hip.call("glowtts_adam_noam", *(t[offset: offset + n].data_ptr() for t in plain), n, st0.cuda().data_ptr(), C.LR, C.B1, C.B2,
               C.EPS, C.DIM, C.WARMUP)
    for i, name in ((0, "p"), (2, "m"), (3, "v"), (4, "e")):
        assert _bits_equal(free[i], held[i]), name
        if i < 4:
            assert _bits_equal(free[i], plain[i]) and _bits_equal(held[i], plain[i]), name
    assert guard.tolist() == [0.0] * 4
    guard[0] = 1.0
    skipped = [t.clone() for t in base]
    _ema_call(G, skipped, offset, n, st0.cuda(), guard, case)
    assert all(_bits_equal(a, b) for a, b in zip(skipped, base))
    assert guard.tolist() == [1.0, 0.0, 0.0, 0.0]


# =============================================================================================== 3. swap
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "off1"])
@pytest.mark.parametrize("n", [1, 5, 4099, 2 ** 21 + 4])
def test_swap_is_exact_and_writes_nothing_outside(G, n, offset):
    gen = torch.Generator(device="cuda").manual_seed(n)
    a0 = torch.randn(n + C.PAD, device="cuda", generator=gen)
    b0 = torch.randn(n + C.PAD, device="cuda", generator=gen)
    a0[:1], b0[n // 2: n // 2 + 1] = NAN, float("inf")                      # data movement: any bit pattern
    a, b = a0.clone(), b0.clone()
    assert a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0
    G.hip.call("glowtts_swap_f32", a[offset:].data_ptr(), b[offset:].data_ptr(), n)
    want_a, want_b = a0.clone(), b0.clone()
    want_a[offset: offset + n], want_b[offset: offset + n] = b0[offset: offset + n], a0[offset: offset + n]
    assert _bits_equal(a, want_a) and _bits_equal(b, want_b)
    # one aligned, one not: the scalar form
    a, b = a0.clone(), b0.clone()
    G.hip.call("glowtts_swap_f32", a.data_ptr(), b[1:].data_ptr(), n)
    assert _bits_equal(a[:n], b0[1: n + 1]) and _bits_equal(b[1: n + 1], a0[:n])
    assert _bits_equal(a[n:], a0[n:]) and _bits_equal(b[:1], b0[:1]) and _bits_equal(b[n + 1:], b0[n + 1:])
    # adjacent halves of one buffer do not overlap; shifted by one element they do
    both = torch.cat([a0[:n], b0[:n]])
    G.hip.call("glowtts_swap_f32", both.data_ptr(), both[n:].data_ptr(), n)
    assert _bits_equal(both, torch.cat([b0[:n], a0[:n]]))
    if n > 1:
        with pytest.raises(RuntimeError, match="overlap"):
            G.hip.call("glowtts_swap_f32", both.data_ptr(), both[n - 1:].data_ptr(), n)


# =============================================================================================== the small model
# (b, t_text, t_mel, text lengths, mel lengths, speakers)
BATCHES = [
    (2, 12, 64, [12, 7], [64, 33], [1, 2]),
    (2, 10, 56, [10, 6], [56, 40], [0, 3]),
    (2, 12, 48, [12, 9], [48, 31], [2, 0]),
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
        batches.append(tuple(t.cuda() for t in (x, xl, y, yl, torch.tensor(spk))))
    return types.SimpleNamespace(hp=hp, sd=sd, batches=batches)


def _bare_model(G, small, sd=None):
    hp = small.hp
    m = G.models.FlowGenerator(
        n_vocab=hp.n_vocab, hidden_channels=hp.hidden_channels, filter_channels=hp.filter_channels,
        filter_channels_dp=hp.filter_channels_dp, out_channels=hp.out_channels, kernel_size=hp.kernel_size,
        n_heads=hp.n_heads, n_layers_enc=hp.n_layers_enc, p_dropout=0.0, n_blocks_dec=hp.n_blocks_dec,
        kernel_size_dec=hp.kernel_size_dec, dilation_rate=hp.dilation_rate, n_block_layers=hp.n_block_layers,
        p_dropout_dec=0.0, n_speakers=hp.n_speakers, gin_channels=hp.gin_channels, n_split=hp.n_split, n_sqz=hp.n_sqz,
        sigmoid_scale=hp.sigmoid_scale, window_size=hp.window_size, mean_only=hp.mean_only, prenet=hp.prenet)
    m.load_state_dict(small.sd if sd is None else sd)
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    return m.cuda().train()


def _model(G, small, **options):
    m = _bare_model(G, small)
    return m, G.optimize.Adam(m.parameters(), scheduler="noam", dim_model=64, warmup_steps=4000, lr=1.0, **options)


# =============================================================================================== 4. the optimizer
@pytest.mark.parametrize("warm", [False, True], ids=["plain", "warmup"])
def test_flat_e_follows_the_fp64_recurrence_over_three_updates(G, small, warm):
    """Three updates with ema_decay = 0.99: flat_e against e_k = e_(k-1) + a_k (p_k - e_(k-1)) in fp64, e_0 = p_0, fed with the
    parameters read back after each update; a_k = 0.01, or max(0.01, 9 / (10 + k)) = 0.9, 9/11, 0.75 with the warm-up.  Bound: the
    per-update bounds of test 1 added up, 16 u sum_k (|e_(k-1)| + |p_k|) per element."""
    model, opt = _model(G, small, ema_decay=0.99, ema_warmup=warm)
    flat = opt._optim
    assert _bits_equal(flat.flat_e, flat.flat_p) and opt.ema_num_updates() == 0
    e = flat.flat_p.cpu().double()
    scale = torch.zeros_like(e)
    for k, batch in enumerate(small.batches):
        G.train.train_batch(model, opt, batch, CLIP)
        p = flat.flat_p.cpu()
        a = C.ema_weight(1.0 - 0.99, int(warm), k)
        scale += e.abs() + p.double().abs()
        e = C.ema_ref(e, p, a)
        assert opt.ema_num_updates() == k + 1
    fig = C.units(flat.flat_e, e, scale)
    moved = float((flat.flat_e - flat.flat_p).abs().max())
    print(f"flat_e after 3 updates, warm-up {warm}: {fig:.2f} u of sum_k (|e| + |p|) (bound {C.E_BOUND:g}); max|e - p| = {moved:.3e}")
    assert fig <= C.E_BOUND
    assert moved > 0.0
    live = torch.zeros(flat.numel_padded, dtype=torch.bool)
    for o, n in flat.slices():
        live[o:o + n] = True
    assert bool((flat.flat_e[~live.cuda()] == 0).all())                      # the padding stays zero


def test_off_means_off(G, small, monkeypatch):
    """Without the option there is no flat_e and no launch of either new entry point; with it the update launch is the EMA entry
    point IN PLACE of glowtts_adam_noam, and nothing else changes."""
    import glow_tts_train.convops as convops
    import glow_tts_train.ops as ops

    launches = []
    real = G.hip.call

    def recording(name, *args, **kw):
        launches.append(name)
        return real(name, *args, **kw)

    monkeypatch.setattr(G.hip, "call", recording)
    for mod in (convops, ops, G.optimize, G.utils, G.train):
        if getattr(mod, "call", None) is real:
            monkeypatch.setattr(mod, "call", recording)
    runs = {}
    for key, options in (("off", {}), ("on", {"ema_decay": 0.99}), ("on+skip", {"ema_decay": 0.99, "skip_nonfinite": True})):
        model, opt = _model(G, small, **options)
        assert (opt._optim.flat_e is None) == (key == "off")
        launches.clear()
        G.train.train_batch(model, opt, small.batches[0], CLIP)
        runs[key] = list(launches)
    assert not [n for n in runs["off"] if "ema" in n or "swap" in n]
    assert runs["off"][-3:] == ["glowtts_clip_grad_value", "glowtts_adam_noam", "glowtts_adam_advance"]
    assert runs["on"][-3:] == ["glowtts_clip_grad_value", "glowtts_adam_noam_ema", "glowtts_adam_advance"]
    assert runs["on+skip"][-3:] == ["glowtts_clip_grad_value_guarded", "glowtts_adam_noam_ema", "glowtts_adam_advance_guarded"]
    swap = {"glowtts_adam_noam": "glowtts_adam_noam_ema"}
    assert sorted(swap.get(n, n) for n in runs["off"]) == sorted(runs["on"])  # (two streams' host order may interleave differently)


# =============================================================================================== 5. with skip_nonfinite
def test_a_skipped_update_leaves_the_average_alone(G, small, monkeypatch):
    """The loss is poisoned as in tests/test_update_guard.py (train.mle_loss times a device scalar).  Clean, poisoned, clean: the
    poisoned update leaves flat_e and ema_num_updates() bit-unchanged, the next clean one moves flat_e."""
    real = G.train.mle_loss
    factor = torch.ones((), device="cuda")
    monkeypatch.setattr(G.train, "mle_loss", lambda *a: real(*a) * factor)
    model, opt = _model(G, small, ema_decay=0.99, ema_warmup=True, skip_nonfinite=True)
    flat = opt._optim
    batch = small.batches[0]
    G.train.train_batch(model, opt, batch, CLIP)
    e1, p1, n1 = flat.flat_e.clone(), flat.flat_p.clone(), opt.ema_num_updates()
    assert n1 == 1 and not _bits_equal(e1, p1)
    factor.fill_(NAN)
    loss = G.train.train_batch(model, opt, batch, CLIP)
    assert not bool(torch.isfinite(loss))
    assert _bits_equal(flat.flat_e, e1) and _bits_equal(flat.flat_p, p1) and opt.ema_num_updates() == n1
    assert flat.guard.tolist() == [0.0, 1.0, 1.0, 1.0]
    factor.fill_(1.0)
    G.train.train_batch(model, opt, batch, CLIP)
    assert not _bits_equal(flat.flat_e, e1) and opt.ema_num_updates() == 2
    assert bool(torch.isfinite(flat.flat_e).all())
    # the second averaged update used the warm-up weight of k = 1, not of k = 2
    want = C.ema_ref(e1.cpu(), flat.flat_p.cpu(), C.ema_weight(0.01, 1, 1))
    fig = C.units(flat.flat_e, want, e1.cpu().double().abs() + flat.flat_p.cpu().double().abs())
    print(f"the update after a skipped one: e {fig:.2f} u (bound {C.E_BOUND:g})")
    assert fig <= C.E_BOUND


# =============================================================================================== 6. swap_ema()
def test_swap_ema_runs_the_model_on_the_averaged_weights(G, small):
    """Inside the scope the parameters are bit-equal to ema_state_dict, after it to what they were; weights_state.epoch advances on
    entry and on exit.  An eval forward inside the scope against the same forward of a fresh model loaded from ema_state_dict: the same
    computation on the same weights run twice, so every output within 2 ulp of its largest element (2**-22 max|x|: the allowance
    tests/test_update_guard.py::_close_to_twin gives two runs of one computation — one rounding per order of summation and side)."""
    model, opt = _model(G, small, ema_decay=0.9)
    flat = opt._optim
    for batch in small.batches[:2]:
        G.train.train_batch(model, opt, batch, CLIP)
    averaged = opt.ema_state_dict(model)
    raw = {k: v.clone() for k, v in model.state_dict().items()}
    assert list(averaged) == list(raw) and any(not torch.equal(averaged[k], raw[k]) for k in raw)
    ptrs = [p.data_ptr() for p in model.parameters()]
    x, xl, y, yl, spk = small.batches[2]

    def forward(m):
        m.eval()
        with torch.no_grad():
            (z, _z_m, _z_logs, logdet, _), (x_m, x_logs, _), (_attn, logw, _logw) = m(x, xl, y, yl, g=spk)
        m.train()
        return {"z": z, "logdet": logdet, "x_m": x_m, "x_logs": x_logs, "logw": logw}

    outside = forward(model)
    epoch = G.hip.weights_state.epoch
    with opt.swap_ema():
        assert G.hip.weights_state.epoch == epoch + 1
        inside_sd = model.state_dict()
        assert all(_bits_equal(inside_sd[k], averaged[k]) for k in averaged)
        assert all(_bits_equal(a, b) for a, b in zip(opt.ema_state_dict(model).values(), averaged.values()))
        assert [p.data_ptr() for p in model.parameters()] == ptrs           # no pointer moved
        inside = forward(model)
        with pytest.raises(RuntimeError, match="swap_ema"):
            opt.step()
    assert G.hip.weights_state.epoch == epoch + 2
    after = model.state_dict()
    assert all(_bits_equal(after[k], raw[k]) for k in raw)
    assert all(_bits_equal(a, b) for a, b in zip(opt.ema_state_dict(model).values(), averaged.values()))
    fresh = forward(_bare_model(G, small, sd=averaged))
    for name, want in fresh.items():
        tol = 2.0 ** -22 * float(want.abs().max())
        err = float((inside[name] - want).abs().max())
        away = float((outside[name] - want).abs().max())
        print(f"eval forward inside swap_ema against a fresh model, {name}: max|diff| {err:.3e} (bound {tol:.3e}); the raw weights "
              f"are {away:.3e} away")
        assert err <= tol, (name, err, tol)
    assert float((outside["z"] - fresh["z"]).abs().max()) > 2.0 ** -22 * float(fresh["z"].abs().max())   # the two weights do differ
    G.train.train_batch(model, opt, small.batches[0], CLIP)                  # and training goes on
    assert opt.ema_num_updates() == 3


# =============================================================================================== 7. train(..., ema_decay=...)
def test_train_writes_the_average_into_every_checkpoint(G, tmp_path, monkeypatch):
    """Two epochs of two updates on the tiny model of tests/test_formats.py, optimizer built by train(): every checkpoint has the two
    new keys, and loading it with ema_decay gives the flat_e the optimizer held when the file was written, bit for bit, and the
    saved num_updates."""
    import json

    from glow_tts_train.config import AudioConfig, ModelConfig, TrainingConfig
    from glow_tts_train.dataset import PhonemeMelCollate
    from helpers import load_golden

    mc = ModelConfig.from_dict(json.loads(str(load_golden("host_ref_checkpoint_expect")["model_config"])))
    cfg = TrainingConfig(model=mc, audio=AudioConfig(mel_channels=8), warmup_steps=10)
    cfg.epochs = 2
    gen = torch.Generator().manual_seed(11)
    items = [(torch.randint(1, 20, (4 + i % 4,), generator=gen, dtype=torch.int32),
              torch.randn(8, 20 + 2 * (i % 5), generator=gen), 0) for i in range(6)]
    loader = torch.utils.data.DataLoader(items, batch_size=3, shuffle=False, drop_last=True,
                                         collate_fn=PhonemeMelCollate(n_frames_per_step=2, pin_memory=True, slots=3))
    held = {}
    real_save = G.checkpoint.save_checkpoint

    def recording(ck, path):
        flat = ck.optimizer._optim
        held[os.path.basename(str(path))] = (flat.flat_e.clone(), flat.flat_p.clone(), ck.optimizer.ema_num_updates())
        return real_save(ck, path)

    monkeypatch.setattr(G.checkpoint, "save_checkpoint", recording)
    last = G.train.train(loader, cfg, tmp_path, ema_decay=0.999, ema_warmup=True)
    assert last == 5 and sorted(held) == ["checkpoint_3.pth", "checkpoint_5.pth"]
    for name, updates in (("checkpoint_3.pth", 2), ("checkpoint_5.pth", 4)):
        flat_e, flat_p, seen = held[name]
        assert seen == updates and not _bits_equal(flat_e, flat_p)
        file = torch.load(tmp_path / name, map_location="cpu", weights_only=True)
        assert set(file) == {"model", "global_step", "learning_rate", "version", "optimizer", "model_ema", "ema"}
        assert file["ema"] == {"decay": 0.999, "warmup": 1, "num_updates": updates}
        back = G.checkpoint.load_checkpoint(tmp_path / name, cfg, ema_decay=0.999, ema_warmup=True)
        assert _bits_equal(back.optimizer._optim.flat_e, flat_e) and _bits_equal(back.optimizer._optim.flat_p, flat_p)
        assert back.optimizer.ema_num_updates() == updates
        synth = G.checkpoint.load_checkpoint(tmp_path / name, cfg, load_optimizer=False, use_ema=True)
        assert all(torch.equal(v.cpu(), file["model_ema"][k]) for k, v in synth.model.state_dict().items())


# =============================================================================================== 8. two data-parallel ranks
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
        torch.manual_seed(1234 + rank)                                       # the ranks start APART: the broadcast makes them one
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
        opt = optimize.Adam(model.parameters(), scheduler="noam", dim_model=64, warmup_steps=4000, lr=1.0)
        red = parallel.FlowBlockReducer(model, opt)
        red.broadcast_parameters(0)
        opt.enable_ema(0.99, warmup=True)                                    # after the broadcast, as its docstring asks
        gen = torch.Generator().manual_seed(500 + rank)
        xl, yl = torch.tensor([12, 7]), torch.tensor([64, 33])
        for _ in range(3):
            x = torch.randint(1, 60, (2, 12), generator=gen) * (torch.arange(12)[None] < xl[:, None])
            y = torch.randn(2, 80, 64, generator=gen) * (torch.arange(64)[None, None] < yl[:, None, None])
            train.train_batch(model, opt, (x.cuda(), xl.cuda(), y.cuda(), yl.cuda(), None), 5.0, red)
        flat = opt._optim
        q.put((rank, flat.flat_p.detach().cpu().numpy().copy(), flat.flat_e.detach().cpu().numpy().copy(), opt.ema_num_updates()))
    finally:
        dist.destroy_process_group()


def test_two_ranks_keep_the_same_average():
    """gloo, both ranks on the one card, FlowBlockReducer, three updates on different data: the ranks hold the same reduced gradient,
    so their parameters are bit-equal (asserted first) — and so are their averages, started after the broadcast."""
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
    (_, p0, e0, n0), (_, p1, e1, n1) = res
    assert n0 == n1 == 3
    same = p0.view(np.int32) == p1.view(np.int32)
    assert bool(same.all()), f"{int((~same).sum())} of {same.size} parameters differ between the ranks"
    assert np.array_equal(e0.view(np.int32)[same], e1.view(np.int32)[same])
    assert not np.array_equal(e0.view(np.int32), p0.view(np.int32))          # the average is not the weights
