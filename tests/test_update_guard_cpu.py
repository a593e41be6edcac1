"""CPU tests of the host side of `skip_nonfinite` (skipping non-finite updates on the device): argument validation of the three
guarded entry points, the optimizer's surface and its `sync_from_device` reconciliation, and the refusals of train.py that
happen before any launch.  No kernel runs here; tests/test_update_guard.py holds the GPU tests."""
import inspect
import types

import pytest
import torch


def test_guarded_entry_points_reject_bad_arguments_without_a_gpu():
    """Null `guard`, other null pointers and a negative `n` are refused on the host, before any launch."""
    from glow_tts_train import _hip

    lib = _hip.load()
    err = lib.glowtts_last_error
    # clip: (g, n, scale, clip, sumsq, guard, stream)
    assert lib.glowtts_clip_grad_value_guarded(1, 4, 1.0, 5.0, 1, None, None) != 0 and b"null pointer" in err()
    assert lib.glowtts_clip_grad_value_guarded(None, 4, 1.0, 5.0, 1, 1, None) != 0 and b"null pointer" in err()
    assert lib.glowtts_clip_grad_value_guarded(1, -1, 1.0, 5.0, 1, 1, None) != 0 and b"glowtts_clip_grad_value_guarded" in err()
    assert lib.glowtts_clip_grad_value_guarded(1, 4, 1.0, -5.0, 1, 1, None) != 0 and b"bad argument" in err()
    assert lib.glowtts_clip_grad_value_guarded(1, 0, 1.0, 5.0, None, 1, None) == 0             # empty: no launch
    # adam: (p, g, m, v, n, state, guard, lr, b1, b2, eps, dim_model, warmup, stream)
    tail = (1.0, 0.9, 0.98, 1e-9, 192.0, 4000.0, None)
    assert lib.glowtts_adam_noam_guarded(1, 1, 1, 1, 4, 1, None, *tail) != 0 and b"null pointer" in err()
    assert lib.glowtts_adam_noam_guarded(1, 1, 1, 1, 4, None, 1, *tail) != 0 and b"null pointer" in err()
    assert lib.glowtts_adam_noam_guarded(1, 1, 1, 1, -4, 1, 1, *tail) != 0 and b"negative size" in err()
    assert lib.glowtts_adam_noam_guarded(1, 1, 1, 1, 0, 1, 1, *tail) == 0
    # advance: (state, guard, lr, dim_model, warmup, stream)
    assert lib.glowtts_adam_advance_guarded(1, None, 1.0, 192.0, 4000.0, None) != 0 and b"null pointer" in err()
    assert lib.glowtts_adam_advance_guarded(None, 1, 1.0, 192.0, 4000.0, None) != 0 and b"null pointer" in err()
    # the fastcall binding carries them with the same arity
    for name, n_args in (("glowtts_clip_grad_value_guarded", 6), ("glowtts_adam_noam_guarded", 13), ("glowtts_adam_advance_guarded", 5)):
        assert len(_hip._SIGNATURES[name]) == n_args and name in _hip.EXPORTED_SYMBOLS


def test_the_option_is_off_by_default_and_keyword_only_on_adam():
    from glow_tts_train import optimize, train

    sig = inspect.signature(optimize.Adam.__init__).parameters
    assert sig["skip_nonfinite"].kind is inspect.Parameter.KEYWORD_ONLY and sig["skip_nonfinite"].default is False
    assert list(sig)[:8] == ["self", "params", "scheduler", "dim_model", "warmup_steps", "lr", "betas", "eps"]     # the reference's
    assert inspect.signature(optimize.FlatAdam.__init__).parameters["skip_nonfinite"].default is False
    for fn in (train.train, train.train_step):
        assert inspect.signature(fn).parameters["skip_nonfinite"].default is False
    for fn in (train.train_batch, train.train_batches):                       # they follow the optimizer: no new argument
        assert "skip_nonfinite" not in inspect.signature(fn).parameters
    ps = [torch.nn.Parameter(torch.randn(5)), torch.nn.Parameter(torch.randn(3, 2))]
    assert optimize.Adam(ps, "noam", 64)._optim.guard is None
    with pytest.raises(TypeError):
        optimize.Adam(ps, "noam", 64, 4000, 1.0, (0.9, 0.98), 1e-9, True)


def _opt(skip, scheduler="noam"):
    from glow_tts_train import optimize

    ps = [torch.nn.Parameter(torch.randn(5)), torch.nn.Parameter(torch.randn(3, 2))]
    return optimize.Adam(ps, scheduler, 64, warmup_steps=10, lr=1.0, skip_nonfinite=skip)


def test_guard_tensor_and_enable():
    opt = _opt(True)
    g = opt._optim.guard
    assert g.shape == (4,) and g.dtype == torch.float32 and g.device == opt._optim.flat_p.device and bool((g == 0).all())
    late = _opt(False)
    late._optim.enable_skip_nonfinite()
    assert late._optim.guard is not None and bool((late._optim.guard == 0).all())
    late._optim.guard[1] = 3.0
    kept = late._optim.guard
    late._optim.enable_skip_nonfinite()                                      # idempotent: the counters are not reset
    assert late._optim.guard is kept and float(kept[1]) == 3.0


def test_state_dict_keeps_torchs_layout_and_not_the_counters():
    a, b = _opt(True), _opt(False)
    a._optim.guard.copy_(torch.tensor([0.0, 2.0, 1.0, 7.0]))
    sa, sb = a.state_dict(), b.state_dict()
    assert sa.keys() == sb.keys() == {"state", "param_groups"}
    assert sa["param_groups"][0].keys() == sb["param_groups"][0].keys()
    assert all(sa["state"][i].keys() == {"step", "exp_avg", "exp_avg_sq"} for i in sa["state"])
    fresh = _opt(True)
    fresh.load_state_dict(sa)                                                # counters restart at zero on resume
    assert bool((fresh._optim.guard == 0).all())


@pytest.mark.parametrize("scheduler", ["noam", None])
def test_sync_from_device_reconciles_a_mirror_that_ran_ahead(scheduler):
    """Three update attempts of which the device skipped one, played by hand on the device state: the mirror is one step ahead
    and comes back to the device's step, with the schedule's rate of THAT step."""
    opt = _opt(True, scheduler)
    twin = _opt(False, scheduler)
    for _ in range(3):
        opt._update_learning_rate()
    for _ in range(2):
        twin._update_learning_rate()
    opt._optim.dev_state.copy_(torch.tensor([3.0, 3.0, 0.0, 0.0]))           # two applied updates
    opt._optim.guard.copy_(torch.tensor([0.0, 1.0, 0.0, 2.0]))
    assert opt.step_num == 4
    counts = opt.sync_from_device()
    assert counts == {"applied": 2, "skipped": 1, "consecutive_skipped": 0}
    assert all(type(v) is int for v in counts.values())
    assert opt.step_num == twin.step_num == 3 and opt.cur_lr == twin.cur_lr
    assert opt._optim.param_groups[0]["lr"] == twin._optim.param_groups[0]["lr"]


def test_sync_from_device_is_a_no_op_on_a_healthy_run_and_without_the_option():
    opt = _opt(False)
    for _ in range(2):
        opt._update_learning_rate()
    opt._optim.dev_state.copy_(torch.tensor([3.0, 3.0, 0.0, 0.0]))
    before = (opt.step_num, opt.cur_lr, opt._optim.param_groups[0]["lr"])
    assert opt.sync_from_device() == {"applied": 0, "skipped": 0, "consecutive_skipped": 0}
    assert (opt.step_num, opt.cur_lr, opt._optim.param_groups[0]["lr"]) == before


def test_sync_keeps_a_pending_imposed_rate_in_the_group():
    """A resumed optimizer's stored rate waits in dev_state[3] for the next APPLIED update; after a skipped one the group's lr
    is that rate again, not the schedule's."""
    opt = _opt(True)
    opt._optim.dev_state[3] = 0.125
    opt._update_learning_rate()                                              # the attempt the device skipped
    opt._optim.guard.copy_(torch.tensor([0.0, 1.0, 1.0, 0.0]))
    assert opt.sync_from_device() == {"applied": 0, "skipped": 1, "consecutive_skipped": 1}
    assert opt.step_num == 1 and opt._optim.param_groups[0]["lr"] == 0.125


def test_train_refuses_before_any_launch():
    from glow_tts_train import train

    cfg = types.SimpleNamespace(grad_clip=5.0)
    plain, guarded = _opt(False), _opt(True)
    with pytest.raises(ValueError, match=r"skip_nonfinite=True\)"):          # says how to build the optimizer
        train.train_step(1, 1, None, plain, cfg, [], skip_nonfinite=True)
    with pytest.raises(ValueError, match="GradScaler"):
        train.train_step(1, 1, None, guarded, cfg, [], scaler=object())
    with pytest.raises(ValueError, match="GradScaler"):
        train.train_batch(None, guarded, (None,) * 5, 5.0, scaler=object())
    assert guarded.step_num == 1 and bool((guarded._optim.guard == 0).all())


@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("guarded", [False, True], ids=["no guard", "guard"])
def test_clip_launch_selects_the_entry_point_and_its_arguments(guarded, scale):
    """optimize.clip_launch, the one place that chooses among the three clip entry points (FlatAdam.clip_grad_value_ and both routes
    of utils.clip_grad_value_ issue what it returns): a guard gives `_guarded` at any scale, else scale != 1 gives `_scaled`, else the
    plain entry, which takes no scale.  The tuples are written out as the call sites spelt them before the selector existed.
    Nothing is launched and `ptr` is the caller's: CPU tensors and their addresses do here."""
    from glow_tts_train import optimize

    g, sumsq = torch.zeros(12), torch.zeros(1)
    guard = torch.zeros(4) if guarded else None
    got = optimize.clip_launch(g, scale, 5, sumsq, guard, lambda t: t.data_ptr())
    if guarded:
        want = ("glowtts_clip_grad_value_guarded", g.data_ptr(), 12, scale, 5.0, sumsq.data_ptr(), guard.data_ptr())
    elif scale == 0.5:
        want = ("glowtts_clip_grad_value_scaled", g.data_ptr(), 12, 0.5, 5.0, sumsq.data_ptr())
    else:
        want = ("glowtts_clip_grad_value", g.data_ptr(), 12, 5.0, sumsq.data_ptr())
    assert got == want
    assert [type(a) for a in got] == [type(a) for a in want]                  # the clip value arrives as a float, n as an int
    from glow_tts_train import _hip

    assert len(got) - 1 == len(_hip._SIGNATURES[got[0]])
