"""CPU tests of the host side of the exponential moving average of the weights (`ema_decay`): argument validation of the two new
entry points, the optimizer's surface on CPU tensors, the checkpoint keys and their round trip, and the refusals that happen
before any launch.  No kernel runs here; tests/test_ema.py holds the GPU tests."""
import inspect
import json
import logging

import pytest
import torch

from helpers import load_golden


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# =============================================================================================== the C ABI
def test_entry_points_reject_bad_arguments_without_a_gpu():
    """Null pointers, a negative `n`, an `ema_rate` outside (0, 1) and overlapping swap operands are refused on the host, before
    any launch; `n == 0` returns 0 without one.  `guard` alone may be NULL."""
    from glow_tts_train import _hip

    lib = _hip.load()
    err = lib.glowtts_last_error
    # (p, g, m, v, e, n, state, guard, lr, b1, b2, eps, dim_model, warmup, ema_rate, ema_warm, ema_t0, stream)
    tail = (1.0, 0.9, 0.98, 1e-9, 192.0, 4000.0, 1e-3, 1, 1.0, None)
    ema = lib.glowtts_adam_noam_ema
    for null_at in (0, 1, 2, 3, 4, 6):
        args = [16, 16, 16, 16, 16, 4, 16, 16]
        args[null_at] = None
        assert ema(*args, *tail) != 0 and b"glowtts_adam_noam_ema: null pointer" in err(), null_at
    assert ema(16, 16, 16, 16, 16, -4, 16, None, *tail) != 0 and b"negative size" in err()
    for rate in (0.0, 1.0, -0.5, float("nan")):
        assert ema(16, 16, 16, 16, 16, 4, 16, None, *tail[:6], rate, 0, 1.0, None) != 0 and b"ema_rate" in err(), rate
    assert ema(16, 16, 16, 16, 16, 0, 16, None, *tail) == 0                   # empty, guard NULL: no launch
    assert ema(16, 16, 16, 16, 16, 0, 16, 16, *tail) == 0
    # (a, b, n, stream)
    swap = lib.glowtts_swap_f32
    assert swap(None, 4096, 4, None) != 0 and b"glowtts_swap_f32: null pointer" in err()
    assert swap(4096, None, 4, None) != 0 and b"null pointer" in err()
    assert swap(4096, 8192, -1, None) != 0 and b"glowtts_swap_f32" in err()
    for a, b, n in ((4096, 4096, 1), (4096, 4096 + 4 * 7, 8), (4096 + 4 * 7, 4096, 8), (4096, 4096 + 4, 1 << 40)):
        assert swap(a, b, n, None) != 0 and b"overlap" in err(), (a, b, n)
    assert swap(4096, 8192, 0, None) == 0
    assert swap(4096, 4096, 0, None) == 0                                     # nothing to exchange, nothing to overlap
    for name, n_args in (("glowtts_adam_noam_ema", 17), ("glowtts_swap_f32", 3)):
        assert len(_hip._SIGNATURES[name]) == n_args and name in _hip.EXPORTED_SYMBOLS


def test_the_bound_of_the_gpu_test_is_four_times_the_fp32_sequence_on_the_cpu():
    """tests/ema_cases.py: E_BOUND is 4 x the worst figure of the kernel's fp32 sequence (numpy, CPU) against fp64 on the inputs and
    cases of the GPU test, rounded up to a power of two — and that figure respects the analytic (1 + 2 a) u."""
    import math

    import ema_cases as C

    worst = 0.0
    for n in C.SIZES:
        p, g, m, v, e, _dead, pad = C.adam_ema_data(n)
        p_new = C.adam_np32(p, g, m, v)
        assert not torch.equal(p_new, p)
        for rate, warm, k in C.EMA_CASES:
            a = C.ema_weight(rate, warm, k)
            got = C.ema_np32(e, p_new, a)
            fig = C.units(got, C.ema_ref(e, p_new, a), e.double().abs() + p_new.double().abs())
            assert fig <= 1.0 + 2.0 * a, (n, a, fig)
            assert bool((got[pad] == 0).all())
            worst = max(worst, fig)
    print(f"fp32 sequence on the CPU against fp64: worst {worst:.2f} u of |e| + |p'|; bound {C.E_BOUND:g} u")
    assert C.E_BOUND == 2.0 ** math.ceil(math.log2(4.0 * worst))
    assert [C.ema_weight(*c) for c in C.EMA_CASES[2:]] == [float(torch.tensor(x, dtype=torch.float32)) for x in (0.9, 0.6, 9.0 / 100010.0)]


# =============================================================================================== the optimizer's surface
def _params():
    gen = torch.Generator().manual_seed(3)
    return [torch.nn.Parameter(torch.randn(5, generator=gen)), torch.nn.Parameter(torch.randn(3, 2, generator=gen))]


def test_the_options_are_off_by_default_and_keyword_only_on_adam():
    from glow_tts_train import checkpoint, optimize, train

    sig = inspect.signature(optimize.Adam.__init__).parameters
    assert list(sig)[:8] == ["self", "params", "scheduler", "dim_model", "warmup_steps", "lr", "betas", "eps"]     # the reference's
    for name, default in (("ema_decay", None), ("ema_warmup", False)):
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY and sig[name].default is default
        assert inspect.signature(optimize.FlatAdam.__init__).parameters[name].default is default
        assert inspect.signature(train.train).parameters[name].default is default
        assert inspect.signature(checkpoint.load_checkpoint).parameters[name].default is default
        for fn in (train.train_batch, train.train_batches, train.train_step, train.GraphedTrainStep.__init__):
            assert name not in inspect.signature(fn).parameters              # they follow the optimizer
    assert inspect.signature(checkpoint.load_checkpoint).parameters["use_ema"].default is False
    opt = optimize.Adam(_params(), "noam", 64)
    assert opt._optim.flat_e is None and opt._optim.ema_decay is None
    for method in ("ema_num_updates", "swap_ema"):
        with pytest.raises(RuntimeError, match="ema_decay"):
            ctx = getattr(opt, method)()
            ctx.__enter__()
    with pytest.raises(RuntimeError, match="ema_decay"):
        opt.ema_state_dict(torch.nn.Linear(2, 2))
    with pytest.raises(TypeError):
        optimize.Adam(_params(), "noam", 64, 4000, 1.0, (0.9, 0.98), 1e-9, False, 0.999)


@pytest.mark.parametrize("decay", [0.0, 1.0, -0.1, 1.5, float("nan")])
def test_a_decay_outside_the_open_unit_interval_raises(decay):
    from glow_tts_train import optimize

    with pytest.raises(ValueError, match="ema_decay"):
        optimize.Adam(_params(), "noam", 64, ema_decay=decay)
    with pytest.raises(ValueError, match="ema_decay"):
        optimize.FlatAdam(_params(), ema_decay=decay)
    opt = optimize.Adam(_params(), "noam", 64)
    with pytest.raises(ValueError, match="ema_decay"):
        opt.enable_ema(decay)
    assert opt._optim.flat_e is None


def test_enable_ema_copies_the_flat_parameters_once():
    from glow_tts_train import optimize

    for built_with in (True, False):
        opt = optimize.Adam(_params(), "noam", 64, ema_decay=0.99 if built_with else None, ema_warmup=built_with)
        flat = opt._optim
        if not built_with:
            opt.enable_ema(0.99, warmup=True)
        assert flat.flat_e is not flat.flat_p and flat.flat_e.data_ptr() != flat.flat_p.data_ptr()
        assert flat.flat_e.shape == (flat.numel_padded,) and _bits_equal(flat.flat_e, flat.flat_p)          # padding included
        assert flat.numel_padded > flat.numel
        assert (flat.ema_decay, flat.ema_warmup, opt.ema_num_updates()) == (0.99, True, 0)
        assert flat._ema_rate == 1.0 - 0.99                                   # fp64: rounded to fp32 once, at the call
        with pytest.raises(RuntimeError, match="already on"):
            opt.enable_ema(0.99)
    # a resumed run: the count continues, and follows the device's step (a skipped update does not advance it)
    opt = optimize.Adam(_params(), "noam", 64)
    opt._optim.dev_state[0] = 41.0
    opt.enable_ema(0.999, num_updates=25)
    assert opt.ema_num_updates() == 25
    opt._optim.dev_state[0] = 43.0
    assert opt.ema_num_updates() == 27
    with pytest.raises(ValueError, match="num_updates"):
        optimize.Adam(_params(), "noam", 64).enable_ema(0.9, num_updates=-1)


def test_state_dict_keeps_torchs_layout_with_and_without_the_average():
    from glow_tts_train import optimize

    a = optimize.Adam(_params(), "noam", 64, warmup_steps=10, ema_decay=0.999, ema_warmup=True)
    b = optimize.Adam(_params(), "noam", 64, warmup_steps=10)
    sa, sb = a.state_dict(), b.state_dict()
    assert sa.keys() == sb.keys() == {"state", "param_groups"}
    assert sa["param_groups"][0].keys() == sb["param_groups"][0].keys()
    assert sa["state"].keys() == sb["state"].keys()
    assert all(sa["state"][i].keys() == {"step", "exp_avg", "exp_avg_sq"} for i in sa["state"])
    # loading a state moves the device's step; the average's count does not move with it
    sb["state"][0]["step"] = sb["state"][1]["step"] = torch.tensor(30.0)
    a._optim.dev_state[0] = 8.0
    assert a.ema_num_updates() == 7
    a.load_state_dict(sb)
    assert float(a._optim.dev_state[0]) == 31.0 and a.ema_num_updates() == 7


def test_ema_state_dict_has_the_models_keys_and_the_averaged_values():
    from glow_tts_train import optimize

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a = torch.nn.Linear(3, 2)
            self.frozen = torch.nn.Linear(2, 2)                               # not handed to the optimizer
            self.register_buffer("count", torch.tensor([3.0, 4.0]))

    net = Net()
    opt = optimize.Adam(net.a.parameters(), "noam", 64, ema_decay=0.9)
    flat = opt._optim
    flat.flat_e.mul_(2.0).add_(1.0)                                           # an average that differs from the weights
    sd, ema = net.state_dict(), opt.ema_state_dict(net)
    assert list(ema) == list(sd) and all(ema[k].shape == sd[k].shape for k in sd)
    for k in ("a.weight", "a.bias"):
        assert torch.equal(ema[k], sd[k] * 2.0 + 1.0), k
    for k in ("frozen.weight", "frozen.bias", "count"):
        assert torch.equal(ema[k], sd[k]) and ema[k].data_ptr() != sd[k].data_ptr(), k
    ema["a.weight"].zero_()                                                   # clones: the average is not touched
    assert bool((flat.flat_e[:6] != 0).all())


def test_step_inside_swap_ema_raises_before_any_launch(monkeypatch):
    """On CPU tensors, with `call` and `ptr` of optimize.py replaced by a recorder: the scope launches one exchange on entry and
    one on exit and moves the weights epoch both times; step(), enable_ema, a nested scope and save_checkpoint raise inside it
    without a launch; entering inside convops.weights_unchanged() raises."""
    from glow_tts_train import _hip, checkpoint, convops, optimize

    launches = []
    monkeypatch.setattr(optimize, "call", lambda name, *a, **k: launches.append(name))
    monkeypatch.setattr(optimize, "ptr", lambda t: None if t is None else t.data_ptr())
    net = torch.nn.Linear(3, 2)
    opt = optimize.Adam(net.parameters(), "noam", 64, ema_decay=0.9)
    epoch = _hip.weights_state.epoch
    with opt.swap_ema() as inside:
        assert inside is opt._optim
        assert launches == ["glowtts_swap_f32"] and _hip.weights_state.epoch == epoch + 1
        with pytest.raises(RuntimeError, match="swap_ema"):
            opt.step()
        with pytest.raises(RuntimeError, match="swap_ema"):
            opt._optim.step()
        with pytest.raises(RuntimeError, match="already on"):
            opt.enable_ema(0.9)
        with pytest.raises(RuntimeError, match="already inside"):
            with opt.swap_ema():
                pass
        with pytest.raises(RuntimeError, match="swap_ema"):
            checkpoint.save_checkpoint(checkpoint.Checkpoint(model=net, optimizer=opt, learning_rate=1.0, global_step=1, version=1),
                                       "/nonexistent/never_written.pth")
        assert launches == ["glowtts_swap_f32"] and opt.step_num == 1
    assert launches == ["glowtts_swap_f32"] * 2 and _hip.weights_state.epoch == epoch + 2
    with pytest.raises(ZeroDivisionError):                                    # an exception inside the scope still swaps back
        with opt.swap_ema():
            1 / 0
    assert launches == ["glowtts_swap_f32"] * 4 and not opt._optim._ema_swapped
    with convops.weights_unchanged():
        with pytest.raises(RuntimeError, match="weights_unchanged"):
            with opt.swap_ema():
                pass
    assert launches == ["glowtts_swap_f32"] * 4
    opt.step()                                                                # outside: the EMA entry point, then the usual advance
    assert launches[4:] == ["glowtts_adam_noam_ema", "glowtts_adam_advance"]
    guarded = optimize.Adam(torch.nn.Linear(3, 2).parameters(), "noam", 64, ema_decay=0.9, skip_nonfinite=True)
    del launches[:]
    guarded.step()
    assert launches == ["glowtts_adam_noam_ema", "glowtts_adam_advance_guarded"]
    plain = optimize.Adam(torch.nn.Linear(3, 2).parameters(), "noam", 64)
    del launches[:]
    plain.step()
    assert launches == ["glowtts_adam_noam", "glowtts_adam_advance"]


# =============================================================================================== checkpoint files
def _tiny_config():
    from glow_tts_train.config import AudioConfig, ModelConfig, TrainingConfig

    e = load_golden("host_ref_checkpoint_expect")
    mc = ModelConfig.from_dict(json.loads(str(e["model_config"])))
    return TrainingConfig(model=mc, audio=AudioConfig(mel_channels=8), warmup_steps=10)


TODAYS_KEYS = {"model", "global_step", "learning_rate", "version", "optimizer"}


def _saved(tmp_path, name, ema):
    """A tiny model and its optimizer on the CPU, written to a file; with `ema` the average is on, differs from the weights and has
    seen 12 updates."""
    from glow_tts_train import checkpoint as C
    from glow_tts_train.models import setup_model

    cfg = _tiny_config()
    torch.manual_seed(4)
    model, opt = setup_model(cfg, use_cuda=False)
    flat = opt._optim
    if ema:
        opt.enable_ema(0.999, warmup=True)
        gen = torch.Generator().manual_seed(9)
        live = torch.zeros(flat.numel_padded, dtype=torch.bool)
        for o, n in flat.slices():
            live[o:o + n] = True
        flat.flat_e.add_(0.01 * torch.randn(flat.numel_padded, generator=gen) * live)
        flat.dev_state[0] = 13.0
        assert opt.ema_num_updates() == 12
    path = tmp_path / name
    C.save_checkpoint(C.Checkpoint(model=model, optimizer=opt, learning_rate=opt.cur_lr, global_step=13, version=1), path)
    return cfg, model, opt, path


def test_checkpoint_keys_with_the_option_off_and_on(tmp_path):
    _, model, opt, off = _saved(tmp_path, "off.pth", ema=False)
    assert set(torch.load(off, weights_only=True)) == TODAYS_KEYS
    _, model, opt, on = _saved(tmp_path, "on.pth", ema=True)
    file = torch.load(on, map_location="cpu", weights_only=True)              # plain torch.load, no allow-list needed
    assert set(file) == TODAYS_KEYS | {"model_ema", "ema"}
    assert file["ema"] == {"decay": 0.999, "warmup": 1, "num_updates": 12}
    assert all(type(v) in (int, float) for v in file["ema"].values())
    assert list(file["model_ema"]) == list(file["model"]) == list(model.state_dict())
    want = opt.ema_state_dict(model)
    assert all(_bits_equal(file["model_ema"][k], want[k]) for k in want)
    assert any(not torch.equal(file["model_ema"][k], file["model"][k]) for k in want)
    assert set(file["optimizer"]) == {"state", "param_groups"}


def test_checkpoint_round_trip_restores_the_average_and_its_count(tmp_path):
    from glow_tts_train import checkpoint as C

    cfg, model, opt, path = _saved(tmp_path, "on.pth", ema=True)
    back = C.load_checkpoint(path, cfg, use_cuda=False, ema_decay=0.999, ema_warmup=True)
    flat, flat0 = back.optimizer._optim, opt._optim
    assert _bits_equal(flat.flat_e, flat0.flat_e) and _bits_equal(flat.flat_p, flat0.flat_p)
    assert not _bits_equal(flat.flat_e, flat.flat_p)
    assert back.optimizer.ema_num_updates() == 12 and (flat.ema_decay, flat.ema_warmup) == (0.999, True)
    # an optimizer passed in that already averages keeps its settings and takes the file's average
    cfg2, model2, opt2, _ = _saved(tmp_path, "other.pth", ema=False)
    opt2.enable_ema(0.9)
    C.load_checkpoint(path, cfg2, model=model2, optimizer=opt2, use_cuda=False, ema_decay=0.999)
    assert opt2._optim.ema_decay == 0.9 and _bits_equal(opt2._optim.flat_e, flat0.flat_e) and opt2.ema_num_updates() == 12
    # without ema_decay the file's extra keys are ignored, as the reference's loader ignores them
    plain = C.load_checkpoint(path, cfg, use_cuda=False)
    assert plain.optimizer._optim.flat_e is None and _bits_equal(plain.optimizer._optim.flat_p, flat0.flat_p)


def test_use_ema_fills_the_model_with_the_averaged_weights(tmp_path):
    from glow_tts_train import checkpoint as C

    cfg, model, opt, path = _saved(tmp_path, "on.pth", ema=True)
    want = opt.ema_state_dict(model)
    for load_optimizer in (False, True):
        back = C.load_checkpoint(path, cfg, load_optimizer=load_optimizer, use_cuda=False, use_ema=True)
        got = back.model.state_dict()
        assert list(got) == list(want) and all(_bits_equal(got[k], want[k]) for k in want)
    _, _, _, off = _saved(tmp_path, "off.pth", ema=False)
    with pytest.raises(KeyError, match="model_ema"):
        C.load_checkpoint(off, cfg, use_cuda=False, use_ema=True)


def test_ema_decay_on_a_file_without_the_average_warns_and_starts_from_the_weights(tmp_path, caplog):
    from glow_tts_train import checkpoint as C

    cfg, model, opt, off = _saved(tmp_path, "off.pth", ema=False)
    with caplog.at_level(logging.WARNING, logger="glow_tts_train.checkpoint"):
        back = C.load_checkpoint(off, cfg, use_cuda=False, ema_decay=0.99)
    assert [r for r in caplog.records if "averaged weights" in r.getMessage()]
    flat = back.optimizer._optim
    assert _bits_equal(flat.flat_e, flat.flat_p) and _bits_equal(flat.flat_p, opt._optim.flat_p)
    assert back.optimizer.ema_num_updates() == 0 and flat.ema_decay == 0.99 and flat.ema_warmup is False
    with pytest.raises(ValueError, match="load_optimizer"):
        C.load_checkpoint(off, cfg, use_cuda=False, load_optimizer=False, ema_decay=0.99)
