"""CPU tests of the parameter groups of the fused update (`lr_scale`, `weight_decay`, `decoupled_weight_decay`, `frozen`): the fp64
reference of tests/group_cases.py against torch.optim.Adam itself, the measured bounds of the GPU test, the argument checks of
glowtts_adam_noam_groups (they run on the host, before any launch), `optimize.named_param_groups`, and FlatAdam's host logic on CPU
tensors (nothing here launches a kernel)."""
import ctypes
import inspect
import math

import pytest
import torch

import group_cases as C


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# =============================================================================================== the reference and the bounds
@pytest.mark.parametrize("name", ["default", "scale0.1", "l2", "decoupled", "scale0.1+l2", "scale0.1+decoupled"])
@pytest.mark.parametrize("state", C.STATES, ids=["imposed", "noam"])
def test_the_fp64_reference_is_torch_adam(name, state):
    """group_ref against ONE step of torch.optim.Adam(weight_decay=, decoupled_weight_decay=) in fp64 on the CPU, its state set to
    (t - 1, m, v) and its rate to rate_t * lr_scale: equal to 1e-13 of |p| + |upd| (the two order their fp64 operations differently)."""
    p, g, m, v = (t.double() for t in C.adam_ema_data(1023)[:4])
    scale, wd, decoupled, _ = (C.f32(x) for x in C.OPTIONS[name])
    q = torch.nn.Parameter(p.clone())
    opt = torch.optim.Adam([q], lr=C.rate_of(state) * scale, betas=(C.f32(C.B1), C.f32(C.B2)), eps=C.f32(C.EPS), weight_decay=wd,
                           decoupled_weight_decay=bool(decoupled))
    opt.state[q] = {"step": torch.tensor(state[0] - 1.0), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
    q.grad = g.clone()
    opt.step()
    want_p, want_m, want_v, upd, _ = C.group_ref(p, g, m, v, state, C.OPTIONS[name])
    tol = 1e-13 * (p.abs() + upd.abs())
    assert bool(((q.detach() - want_p).abs() <= tol).all())
    assert bool(((opt.state[q]["exp_avg"] - want_m).abs() <= 1e-13 * (m.abs() + g.abs() + 1)).all())
    assert bool(((opt.state[q]["exp_avg_sq"] - want_v).abs() <= 1e-13 * (want_v.abs() + 1)).all())
    if wd != 0.0:                                                            # the decay does something, and the two forms differ
        plain = C.group_ref(p, g, m, v, state, (scale, 0.0, 0, 0))[0]
        assert float((want_p - plain).abs().max()) > (1e-6 if state[3] > 0 else 1e-9)     # (the schedule's rate at s = 123456 is 2e-6)


def test_the_bounds_of_the_gpu_test_are_four_times_the_fp32_sequence_on_the_cpu():
    """tests/group_cases.py: MEASURED is what the kernel's fp32 sequence (numpy, CPU) shows against fp64 over the sizes, states and
    option sets of the GPU test, to the two decimals written there; BOUNDS is 4 x that, rounded up to a power of two."""
    worst = C.measure()
    for form, figs in worst.items():
        print(f"fp32 sequence on the CPU against fp64, {form}: m {figs[0]:.2f} u, v {figs[1]:.2f} u, p {figs[2]:.2f} u; "
              f"bounds {C.BOUNDS[form]}")
    assert set(worst) == set(C.MEASURED) == {"plain", "l2", "decoupled"}
    for form, figs in worst.items():
        assert all(abs(a - b) <= 0.0051 for a, b in zip(figs, C.MEASURED[form])), (form, figs, C.MEASURED[form])
        assert C.BOUNDS[form] == tuple(2.0 ** math.ceil(math.log2(4.0 * f)) for f in figs)


def test_the_fp32_sequence_keeps_padding_at_zero_and_a_zero_rate_leaves_p():
    p, g, m, v, _e, _dead, pad = C.adam_ema_data(4224)
    for name, option in C.OPTIONS.items():
        if name in C.FROZEN:
            continue
        got_p, got_m, got_v = C.group_np32(p, g, m, v, C.STATES[0], option)
        assert bool((got_p[pad] == 0).all()) and bool((got_m[pad] == 0).all()) and bool((got_v[pad] == 0).all()), name
    got_p, got_m, _ = C.group_np32(p, g, m, v, C.STATES[0], C.OPTIONS["scale0"])
    assert _bits_equal(got_p, p) and not _bits_equal(got_m, m)


# =============================================================================================== the C ABI
def test_the_grouped_entry_point_rejects_bad_arguments_without_a_gpu():
    """Every refusal of include/glowtts_hip.h (adam_groups) comes from the host, before any launch: null pointers, n_groups outside
    1 .. GLOWTTS_MAX_PARAM_GROUPS, ends that do not ascend or do not end at n, a negative or non-finite option, a flag that is neither
    0 nor 1, an ema_rate outside (0, 1) when there is an average.  e and guard may be NULL; n == 0 returns 0 without a launch."""
    from glow_tts_train import _hip

    lib = _hip.load()
    err = lib.glowtts_last_error
    fn = lib.glowtts_adam_noam_groups
    assert _hip.CONSTANTS["GLOWTTS_MAX_PARAM_GROUPS"] == 8 and len(_hip._SIGNATURES["glowtts_adam_noam_groups"]) == 20

    def call(ptrs=None, n=128, ends=(64, 128), opts=((1.0, 0.0, 0, 0), (1.0, 0.01, 1, 0)), n_groups=None, ema_rate=1e-3,
             null_table=None):
        # (p, g, m, v, e, n, state, guard, lr, b1, b2, eps, dim_model, warmup, ema_rate, ema_warm, ema_t0, group_end, group_opts, n_groups, stream)
        ptrs = [16, 16, 16, 16, 16, 16, 16] if ptrs is None else ptrs          # p, g, m, v, e, state, guard
        end = (ctypes.c_int64 * max(len(ends), 1))(*ends)
        flat = [float(x) for o in opts for x in o]
        opt = (ctypes.c_float * max(len(flat), 1))(*flat)
        tables = [ctypes.addressof(end), ctypes.addressof(opt)]
        if null_table is not None:
            tables[null_table] = None
        return fn(*ptrs[:5], n, ptrs[5], ptrs[6], 1.0, 0.9, 0.98, 1e-9, 192.0, 4000.0, ema_rate, 1, 1.0, *tables,
                  len(ends) if n_groups is None else n_groups, None)

    for null_at in (0, 1, 2, 3, 5):
        ptrs = [16] * 7
        ptrs[null_at] = None
        assert call(ptrs) != 0 and b"glowtts_adam_noam_groups: null pointer" in err(), null_at
    for null_table in (0, 1):
        assert call(null_table=null_table) != 0 and b"null pointer" in err()
    assert call(n=-128) != 0 and b"negative size" in err()
    for n_groups in (0, -1, 9):
        assert call(n_groups=n_groups) != 0 and b"GLOWTTS_MAX_PARAM_GROUPS" in err() and b"1 .. 8" in err(), n_groups
    nine = tuple(64 * (k + 1) for k in range(9))
    assert call(n=576, ends=nine, opts=((1.0, 0.0, 0, 0),) * 9) != 0 and b"1 .. 8" in err()
    assert call(ends=(128, 64)) != 0 and b"ascend" in err()
    assert call(ends=(-1, 128)) != 0 and b"ascend" in err()
    assert call(ends=(64, 127)) != 0 and b"end at n" in err()
    assert call(ends=(64, 192)) != 0 and b"end at n" in err()
    for bad, what in (((-0.5, 0.0, 0, 0), b"lr_scale < 0"), ((1.0, -1e-3, 0, 0), b"weight_decay < 0"),
                      ((float("nan"), 0.0, 0, 0), b"non-finite"), ((1.0, float("inf"), 0, 0), b"non-finite"),
                      ((1.0, 0.0, float("nan"), 0), b"non-finite"), ((1.0, 0.0, 0, float("inf")), b"non-finite"),
                      ((1.0, 0.0, 2, 0), b"0 or 1"), ((1.0, 0.0, 0, 0.5), b"0 or 1"), ((1.0, 0.0, -1, 0), b"0 or 1")):
        for at in (0, 1):
            opts = [(1.0, 0.0, 0, 0)] * 2
            opts[at] = bad
            assert call(opts=opts) != 0 and what in err() and b"glowtts_adam_noam_groups" in err(), (bad, at, err())
    for rate in (0.0, 1.0, float("nan")):
        assert call(ema_rate=rate) != 0 and b"ema_rate" in err()
    # nothing to do: no launch (and so no GPU needed) — n == 0 with empty groups, e and guard NULL, an unused ema_rate
    assert call(n=0, ends=(0, 0)) == 0
    assert call(ptrs=[16, 16, 16, 16, None, 16, None], n=0, ends=(0,), opts=((1.0, 0.0, 0, 1),), ema_rate=0.0) == 0


# =============================================================================================== named_param_groups
class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.encoder = torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.Linear(4, 2))
        self.proj = torch.nn.Linear(2, 2)
        self.decoder = torch.nn.Sequential(torch.nn.Linear(2, 70), torch.nn.Linear(70, 1))


def _names(model, groups):
    by_id = {id(p): n for n, p in model.named_parameters()}
    return [[by_id[id(p)] for p in g["params"]] for g in groups]


def test_named_param_groups_longest_prefix_first_appearance_and_default():
    from glow_tts_train import optimize

    net = _Net()
    rules = {"decoder.": {"lr_scale": 0.5, "weight_decay": 1e-2, "decoupled_weight_decay": True}, "encoder.": {"frozen": True},
             "encoder.1.": {"lr_scale": 0.1}}
    groups = optimize.named_param_groups(net, rules, default={"weight_decay": 1e-3})
    # order of first appearance in named_parameters(), not the order of the rules; the longest prefix wins; unmatched -> default
    assert _names(net, groups) == [["encoder.0.weight", "encoder.0.bias"], ["encoder.1.weight", "encoder.1.bias"],
                                   ["proj.weight", "proj.bias"],
                                   ["decoder.0.weight", "decoder.0.bias", "decoder.1.weight", "decoder.1.bias"]]
    assert [{k: v for k, v in g.items() if k != "params"} for g in groups] == [
        {"frozen": True}, {"lr_scale": 0.1}, {"weight_decay": 1e-3}, rules["decoder."]]
    assert _names(net, optimize.named_param_groups(net, None)) == [[n for n, _ in net.named_parameters()]]
    assert optimize.named_param_groups(net, {}, default=None)[0].keys() == {"params"}
    with pytest.raises(ValueError, match="dekoder"):
        optimize.named_param_groups(net, {"encoder.": {}, "dekoder.": {"frozen": True}})
    # a prefix that does match names, but loses every one of them to longer prefixes, is refused in its own words
    with pytest.raises(ValueError, match=r"under \['encoder\.'\] is taken by a longer prefix"):
        optimize.named_param_groups(net, {"encoder.": {}, "encoder.0.": {}, "encoder.1.": {}})
    # interleaving rules are allowed here (the data-parallel reducer is what refuses them): one group per rule all the same
    by_kind = optimize.named_param_groups(net, {"encoder.0.bias": {"weight_decay": 0.0}}, default={"weight_decay": 1e-2})
    assert _names(net, by_kind)[1] == ["encoder.0.bias"] and len(by_kind) == 2
    assert "FlowBlockReducer" in optimize.named_param_groups.__doc__


def test_param_rules_is_keyword_only_on_setup_model_and_reaches_train_and_load_checkpoint():
    from glow_tts_train import checkpoint, models, train

    assert inspect.signature(models.setup_model).parameters["param_rules"].kind is inspect.Parameter.KEYWORD_ONLY
    for fn in (models.setup_model, train.train, checkpoint.load_checkpoint):
        assert inspect.signature(fn).parameters["param_rules"].default is None
    names = list(inspect.signature(models.setup_model).parameters)
    assert names == ["config", "model", "optimizer", "model_factory", "optimizer_factory", "create_optimizer", "use_cuda", "param_rules"]


# =============================================================================================== FlatAdam on CPU tensors
SIZES = (1, 65, 4099)
GROUPS = ({}, {"lr_scale": 0.1, "weight_decay": 1e-2}, {"weight_decay": 1e-2, "decoupled_weight_decay": True})


def _params(sizes=SIZES, seed=3):
    gen = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(n, generator=gen)) for n in sizes]


def _grouped(options=GROUPS, sizes=SIZES, seed=3):
    return [{"params": [p], **o} for p, o in zip(_params(sizes, seed), options)]


def test_refusals_at_construction():
    from glow_tts_train import optimize

    nine = [{"params": [p]} for p in _params((2,) * 9)]
    with pytest.raises(ValueError, match="at most 8"):
        optimize.FlatAdam(nine)
    optimize.FlatAdam(nine[:8])
    for bad in ({"betas": (0.8, 0.98)}, {"eps": 1e-6}):
        with pytest.raises(ValueError, match="shared"):
            optimize.FlatAdam(_grouped(({}, bad, {})))
    for bad in ({"lr_scale": -0.1}, {"weight_decay": -1e-2}, {"lr_scale": float("nan")}, {"weight_decay": float("inf")}):
        with pytest.raises(ValueError, match="finite and >= 0"):
            optimize.FlatAdam(_grouped(({}, bad, {})))
    with pytest.raises(ValueError, match="lr_scale"):
        optimize.FlatAdam(_grouped(({}, {"lr": 0.5}, {})))
    with pytest.raises(ValueError, match="at most 8"):
        optimize.Adam(nine, scheduler="noam", dim_model=192)


def test_group_ranges_fall_out_of_the_offsets():
    from glow_tts_train import optimize

    opt = optimize.FlatAdam(_grouped())
    assert opt.offsets == [0, 64, 192] and opt.numel_padded == 192 + 4160
    assert opt.group_ends == [64, 192, 4352] and list(opt._group_end) == opt.group_ends
    assert all(e % 64 == 0 for e in opt.group_ends)
    two = optimize.FlatAdam([{"params": _params((65, 1))}, {"params": _params((3,)), "frozen": True}])
    assert two.group_ends == [192, 256]
    assert optimize.FlatAdam(_params()).group_ends == [4352]
    assert opt._all_default() is False and optimize.FlatAdam(_grouped(({}, {}, {})))._all_default() is True
    assert optimize.FlatAdam(_grouped(({}, {"decoupled_weight_decay": True, "lr_scale": 1.0, "frozen": False}, {})))._all_default()
    # the options are read at every step: editing a group is seen
    opt.param_groups[1]["weight_decay"] = -1.0
    with pytest.raises(ValueError, match="group 1"):
        opt._group_options()


def test_state_dict_groups_are_torchs():
    """The group lists (indices, group-major) and every torch key equal torch.optim.Adam's built from the same groups; `lr_scale` /
    `frozen` appear only when some group uses one, and then in every group."""
    from glow_tts_train import optimize

    torch_groups = [{k: v for k, v in g.items() if k not in ("lr_scale", "frozen")} for g in _grouped()]
    torch_groups[1]["lr"] = 0.5 * 0.1
    ref = torch.optim.Adam(torch_groups, lr=0.5, betas=(0.9, 0.98), eps=1e-9).state_dict()["param_groups"]
    got = optimize.FlatAdam(_grouped(), lr=0.5).state_dict()["param_groups"]
    assert [g["params"] for g in got] == [g["params"] for g in ref] == [[0], [1], [2]]
    assert [{k: v for k, v in g.items() if k not in ("lr_scale", "frozen")} for g in got] == ref
    assert [(g["lr_scale"], g["frozen"]) for g in got] == [(1.0, False), (0.1, False), (1.0, False)]
    # decay alone is torch's own key: no new key in the file
    plain = optimize.FlatAdam(_grouped(({}, {"weight_decay": 1e-2}, {"lr_scale": 1.0})), lr=0.5).state_dict()["param_groups"]
    assert all(g.keys() == ref[0].keys() for g in plain)
    two = optimize.FlatAdam([{"params": _params((65, 1))}, {"params": _params((3, 2)), "frozen": True}]).state_dict()
    assert [g["params"] for g in two["param_groups"]] == [[0, 1], [2, 3]] and sorted(two["state"]) == [0, 1, 2, 3]
    assert [g["frozen"] for g in two["param_groups"]] == [False, True]


def test_the_single_default_groups_state_dict_is_key_for_key_todays():
    """One group at defaults, built from a parameter list or from one dict: exactly the keys, their order and the values of
    torch.optim.Adam's own state_dict for this torch."""
    from glow_tts_train import optimize

    ref = torch.optim.Adam(_params(), lr=0.5, betas=(0.9, 0.98), eps=1e-9).state_dict()["param_groups"]
    for params in (_params(), [{"params": _params()}]):
        got = optimize.FlatAdam(params, lr=0.5).state_dict()
        assert list(got) == ["state", "param_groups"] and len(got["param_groups"]) == 1
        assert list(got["param_groups"][0].items()) == list(ref[0].items())
        assert all(list(s) == ["step", "exp_avg", "exp_avg_sq"] for s in got["state"].values())


def _fill_moments(opt, seed):
    gen = torch.Generator().manual_seed(seed)
    opt.flat_m.copy_(torch.randn(opt.numel_padded, generator=gen))
    opt.flat_v.copy_(torch.rand(opt.numel_padded, generator=gen))
    opt.dev_state[0] = 8.0


def test_round_trip_into_a_twin():
    from glow_tts_train import optimize

    options = GROUPS + ({"frozen": True},)
    a = optimize.Adam(_grouped(options, SIZES + (7,)), scheduler="noam", dim_model=192, warmup_steps=10, lr=1.0)
    _fill_moments(a._optim, 1)
    for g in a._optim.param_groups:
        g["lr"] = 0.02 * g.get("lr_scale", 1.0)
    sd = a.state_dict()
    assert [g["lr"] for g in sd["param_groups"]] == [0.02, 0.002, 0.02, 0.02]
    b = optimize.Adam(_grouped(({}, {}, {}, {}), SIZES + (7,), seed=4), scheduler="noam", dim_model=192, warmup_steps=10, lr=1.0)
    b.load_state_dict(sd)
    fa, fb = a._optim, b._optim
    for (o, n) in fa.slices():
        assert _bits_equal(fa.flat_m[o:o + n], fb.flat_m[o:o + n]) and _bits_equal(fa.flat_v[o:o + n], fb.flat_v[o:o + n])
    assert fb._group_options() == fa._group_options() == [(1.0, 0.0, False, False), (0.1, 1e-2, False, False),
                                                          (1.0, 1e-2, True, False), (1.0, 0.0, False, True)]
    assert [g["lr"] for g in fb.param_groups] == [g["lr"] for g in sd["param_groups"]]
    assert float(fb.dev_state[0]) == 8.0 and float(fb.dev_state[3]) == pytest.approx(0.02, rel=1e-7)
    back = b.state_dict()
    assert back["param_groups"] == sd["param_groups"]
    # several groups in the file, another count here: refused
    with pytest.raises(ValueError, match="4 parameter groups, the optimizer has 3"):
        optimize.FlatAdam([{"params": _params((1, 65))}, {"params": _params((4099,))}, {"params": _params((7,))}]).load_state_dict(sd)
    # as many groups and parameters, but other group sizes: the file's options would land on other parameters — refused, as torch does
    split = optimize.FlatAdam([{"params": _params((1, 65))}, {"params": _params((4099,))}]).state_dict()
    assert [g["params"] for g in split["param_groups"]] == [[0, 1], [2]]
    other = optimize.FlatAdam([{"params": _params((1,))}, {"params": _params((65, 4099))}])
    with pytest.raises(ValueError, match=r"groups of \[2, 1\] parameters, the optimizer's have \[1, 2\]"):
        other.load_state_dict(split)
    assert other._group_options() == [(1.0, 0.0, False, False)] * 2


@pytest.mark.parametrize("scheduler", ["noam", None])
def test_a_file_without_the_new_keys_resets_them_when_the_group_counts_match(scheduler):
    """state_dict() leaves `lr_scale` / `frozen` out when no group uses one (groups that differ in weight_decay only; every file
    from before the groups).  Loaded into an optimizer with AS MANY groups, the file's options win, so the absent keys say 1.0 /
    False: the optimizer's own lr_scale must not survive and divide the file's rate, which was saved at scale 1.  The imposed
    base rate is the file's 0.0125 (dev_state[3] under the schedule, base_lr with a constant rate), every mirror reads it, and
    the group options are the file's."""
    from glow_tts_train import optimize

    def build(options, sizes, seed):
        return optimize.Adam(_grouped(options, sizes, seed), scheduler=scheduler, dim_model=192, warmup_steps=10, lr=1.0)

    def imposed(opt):
        flat = opt._optim
        if scheduler == "noam":
            assert flat.base_lr == 1.0
            return float(flat.dev_state[3])
        assert float(flat.dev_state[3]) == 0.0
        return flat.base_lr

    # ---- two groups that differ in weight_decay only, into {lr_scale 0.1, frozen}, {lr_scale 0.5}
    base = build(({"weight_decay": 1e-2}, {}), SIZES[:2], 11)
    _fill_moments(base._optim, 4)
    for g in base._optim.param_groups:
        g["lr"] = 0.0125
    sd = base.state_dict()
    assert all("lr_scale" not in g and "frozen" not in g for g in sd["param_groups"])
    new = build(({"lr_scale": 0.1, "frozen": True}, {"lr_scale": 0.5}), SIZES[:2], 12)
    new.load_state_dict(sd)
    assert new._optim._group_options() == [(1.0, 1e-2, False, False), (1.0, 0.0, False, False)]
    assert imposed(new) == pytest.approx(0.0125, rel=1e-7)
    assert [g["lr"] for g in new._optim.param_groups] == [0.0125, 0.0125]
    assert new.state_dict()["param_groups"] == sd["param_groups"]
    # ---- the pre-change one-group file into ONE group built with lr_scale 0.5
    old = optimize.Adam(_params(), scheduler=scheduler, dim_model=192, warmup_steps=10, lr=1.0)
    _fill_moments(old._optim, 5)
    old._optim.param_groups[0]["lr"] = 0.0125
    sd = old.state_dict()
    one = optimize.Adam([{"params": _params(seed=13), "lr_scale": 0.5}], scheduler=scheduler, dim_model=192, warmup_steps=10, lr=1.0)
    one.load_state_dict(sd)
    assert one._optim._group_options() == [(1.0, 0.0, False, False)] and one._optim._all_default()
    assert imposed(one) == pytest.approx(0.0125, rel=1e-7) and one._optim.param_groups[0]["lr"] == 0.0125
    assert one.state_dict()["param_groups"] == sd["param_groups"]


def test_the_mirrors_follow_the_imposed_base_rate_not_the_files_other_entries():
    """A file whose groups' `lr` entries disagree with their scales (edited by hand): the base rate comes from the first live group,
    and every mirror is that rate times the group's scale — what the kernel applies."""
    from glow_tts_train import optimize

    a = optimize.Adam(_grouped(), scheduler=None, dim_model=192, lr=1.0)
    sd = a.state_dict()
    for g, lr in zip(sd["param_groups"], (0.02, 0.5, 0.7)):
        g["lr"] = lr
    b = optimize.Adam(_grouped(seed=14), scheduler=None, dim_model=192, lr=1.0)
    b.load_state_dict(sd)
    assert b._optim.base_lr == 0.02 and [g["lr"] for g in b._optim.param_groups] == [0.02, 0.02 * 0.1, 0.02]


def test_a_pre_change_single_group_dict_loads_into_three_groups():
    """What this package wrote before parameter groups (one group, torch's keys only) loads into a three-group optimizer: moments by
    index, the file's rate imposed as the BASE rate, the host mirrors scaled per group, and the new options untouched."""
    from glow_tts_train import optimize

    old = optimize.Adam(_params(), scheduler="noam", dim_model=192, warmup_steps=10, lr=1.0)
    _fill_moments(old._optim, 2)
    old._optim.param_groups[0]["lr"] = 0.0125
    sd = old.state_dict()
    assert len(sd["param_groups"]) == 1 and "lr_scale" not in sd["param_groups"][0] and "frozen" not in sd["param_groups"][0]
    new = optimize.Adam(_grouped(seed=5), scheduler="noam", dim_model=192, warmup_steps=10, lr=1.0)
    new.load_state_dict(sd)
    fo, fn = old._optim, new._optim
    assert fn.offsets == fo.offsets
    assert all(_bits_equal(fn.flat_m[o:o + n], fo.flat_m[o:o + n]) and _bits_equal(fn.flat_v[o:o + n], fo.flat_v[o:o + n])
               for o, n in fn.slices())
    assert fn._group_options() == [(1.0, 0.0, False, False), (0.1, 1e-2, False, False), (1.0, 1e-2, True, False)]
    assert float(fn.dev_state[3]) == pytest.approx(0.0125, rel=1e-7) and float(fn.dev_state[0]) == 8.0
    assert [g["lr"] for g in fn.param_groups] == [0.0125, 0.0125 * 0.1, 0.0125]
    # and into ONE group, as before the change
    same = optimize.Adam(_params(seed=6), scheduler="noam", dim_model=192, warmup_steps=10, lr=1.0)
    same.load_state_dict(sd)
    assert float(same._optim.dev_state[3]) == pytest.approx(0.0125, rel=1e-7) and same._optim.param_groups[0]["lr"] == 0.0125


def test_the_imposed_rate_is_a_base_rate_when_group_0_is_frozen():
    """Groups (frozen, lr_scale 0, lr_scale 0.25, default) saved with a rate of 0.02: the first live group with a rate is group 2,
    whose stored lr is 0.02 * 0.25 — the rate imposed on the next update is 0.02, under the schedule (dev_state[3]) and without
    one (base_lr)."""
    from glow_tts_train import optimize

    options = ({"frozen": True}, {"lr_scale": 0.0}, {"lr_scale": 0.25}, {})
    for scheduler in ("noam", None):
        a = optimize.Adam(_grouped(options, (3, 5, 7, 9)), scheduler=scheduler, dim_model=192, warmup_steps=10, lr=1.0)
        _fill_moments(a._optim, 3)
        for g in a._optim.param_groups:
            g["lr"] = 0.02 * g.get("lr_scale", 1.0)
        sd = a.state_dict()
        assert [g["lr"] for g in sd["param_groups"]] == [0.02, 0.0, 0.005, 0.02]
        b = optimize.Adam(_grouped(options, (3, 5, 7, 9), seed=9), scheduler=scheduler, dim_model=192, warmup_steps=10, lr=1.0)
        b.load_state_dict(sd)
        if scheduler == "noam":
            assert float(b._optim.dev_state[3]) == pytest.approx(0.02, rel=1e-7) and b._optim.base_lr == 1.0
        else:
            assert b._optim.base_lr == 0.02 and float(b._optim.dev_state[3]) == 0.0


def test_the_wrappers_host_mirror_scales_every_groups_rate():
    from glow_tts_train import optimize

    opt = optimize.Adam(_grouped(), scheduler="noam", dim_model=192, warmup_steps=10, lr=1.0)
    scales = [1.0, 0.1, 1.0]
    assert [g["lr"] for g in opt._optim.param_groups] == [opt.cur_lr * s for s in scales]
    for _ in range(3):
        opt._update_learning_rate()
        assert [g["lr"] for g in opt._optim.param_groups] == [opt.cur_lr * s for s in scales]
    const = optimize.Adam(_grouped(), scheduler=None, dim_model=192, lr=0.5)
    assert [g["lr"] for g in const._optim.param_groups] == [0.5, 0.5 * 0.1, 0.5]
