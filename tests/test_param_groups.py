"""GPU tests (-m gpu) of the parameter groups of the fused update: glowtts_adam_noam_groups, and `lr_scale` / `weight_decay` /
`decoupled_weight_decay` / `frozen` through optimize.FlatAdam, optimize.Adam, checkpoint and one training step.

Kernel level, on buffers the test fills itself: a group at defaults is bit-equal to glowtts_adam_noam / _guarded / _ema run on clones
of that range alone; a frozen range, the gradient, the state and everything outside [offset, offset + n) are bit-unchanged; a set
guard leaves everything alone; the other groups meet the fp64 reference of tests/group_cases.py inside its measured bounds (m / v /
p: 8 / 16 / 64 u plain and decoupled, 16 / 16 / 64 u L2; the average 16 u of |e| + |p'|, tests/ema_cases.py); elements with
p = g = m = v = 0 stay exactly zero under both decays.

Optimizer level: thirty updates of three groups against torch.optim.Adam in fp64 with the same groups, bound per tensor
max(4 e_ref, 16 u max|p|) as in tests/test_train_tail.py::_trajectory — this is the test that fails without the feature (the
decayed groups come out as plain Adam); a frozen fourth group; "defaults launch what they launched before"; a NaN in a frozen
group's gradient still skips the update; a checkpoint round trip.  Step level: the small model of tests/test_grad_accum.py with
its encoder frozen."""
import ctypes
import types

import pytest
import torch

import ema_cases as E
import group_cases as C

pytestmark = pytest.mark.gpu

CLIP = 5.0
NAN = float("nan")
EMA_CASE = (0.1, 0, 3)                        # (ema_rate, ema_warm, k): a = 0.1


@pytest.fixture(scope="module")
def G():
    from glow_tts_train import _hip, checkpoint, convops, models, optimize, parallel, train, utils

    _hip.load()
    return types.SimpleNamespace(hip=_hip, checkpoint=checkpoint, convops=convops, models=models, optimize=optimize,
                                 parallel=parallel, train=train, utils=utils)


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# =============================================================================================== 1. the raw kernel
EIGHT = tuple(64 * (k + 1) for k in range(8))
# (n, ends): see the table in the docstring of test_groups_update_raw
SHAPES = [(5, (5,)), (5, (2, 5)), (192, (64, 128, 192)), (1023, (1, 513, 1023)), (4224, (64, 4160, 4224)), (196, (66, 128, 196)),
          (2 ** 21 + 192, (2 ** 20 + 64, 2 ** 21 + 64, 2 ** 21 + 192)), (512, EIGHT)]
# option sets per group (names of group_cases.OPTIONS), by number of groups: every set appears, frozen first, in the middle and last
LAYOUTS = {
    1: [("default",), ("scale0.1",), ("scale0",), ("l2",), ("decoupled",), ("frozen",)],
    2: [("default", "l2"), ("frozen", "decoupled"), ("scale0.1", "frozen"), ("scale0", "default")],
    3: [("default", "l2", "decoupled"), ("frozen", "scale0.1", "default"), ("l2", "frozen", "scale0"),
        ("decoupled", "default", "frozen"), ("scale0.1+l2", "scale0.1+decoupled", "frozen+decay")],
    8: [("default", "scale0.1", "scale0", "l2", "decoupled", "frozen", "scale0.1+l2", "scale0.1+decoupled"),
        ("frozen", "scale0.1+l2", "scale0.1+decoupled", "default", "scale0.1", "scale0", "l2", "frozen+decay"),
        ("frozen",) * 8],
}
LARGE_LAYOUTS = [("default", "l2", "decoupled"), ("decoupled", "frozen", "l2")]


def _tables(ends, names):
    end = (ctypes.c_int64 * len(ends))(*ends)
    opts = (ctypes.c_float * (4 * len(names)))(*[float(x) for name in names for x in C.OPTIONS[name]])
    return end, opts


def _groups_call(G, bufs, offset, n, ends, names, state, guard=None, with_e=True, n_groups=None, case=EMA_CASE):
    """glowtts_adam_noam_groups on [offset, offset + n) of bufs = [p, g, m, v, e]; the two host tables die when this returns."""
    p, g, m, v, e = (b[offset: offset + n] for b in bufs)
    end, opts = _tables(ends, names)
    rate, warm, k = case
    G.hip.call("glowtts_adam_noam_groups", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), e.data_ptr() if with_e else None,
               n, state.data_ptr(), None if guard is None else guard.data_ptr(), C.LR, C.B1, C.B2, C.EPS, C.DIM, C.WARMUP, rate, warm,
               state_t(state) - k, ctypes.addressof(end), ctypes.addressof(opts), len(ends) if n_groups is None else n_groups)
    end[:] = [-7] * len(end)                                                 # nothing of the tables is read after the call


def state_t(state):
    return float(state[0])


def _plain_call(G, bufs, lo, n, state, guard, with_e, case=EMA_CASE):
    """The pre-existing entry point of the same form on [lo, lo + n) alone."""
    p, g, m, v, e = (b[lo: lo + n] for b in bufs)
    four = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr())
    rates = (C.LR, C.B1, C.B2, C.EPS, C.DIM, C.WARMUP)
    if with_e:
        G.hip.call("glowtts_adam_noam_ema", *four, e.data_ptr(), n, state.data_ptr(), None if guard is None else guard.data_ptr(),
                   *rates, case[0], case[1], state_t(state) - case[2])
    elif guard is not None:
        G.hip.call("glowtts_adam_noam_guarded", *four, n, state.data_ptr(), guard.data_ptr(), *rates)
    else:
        G.hip.call("glowtts_adam_noam", *four, n, state.data_ptr(), *rates)


@pytest.fixture(scope="module")
def base():
    """[p, g, m, v, e] on the device per n, made once and never written; the tests work on clones."""
    out = {}
    for n in sorted({n for n, _ in SHAPES} | {576}):
        out[n] = [t.cuda() for t in C.adam_ema_data(n)[:5]]
        assert all(t.data_ptr() % 16 == 0 for t in out[n])
    return out


def _check_layout(G, base_n, n, offset, ends, names, state, worst):
    """One grouped launch with the average (guard NULL) checked group by group; returns the buffers it left."""
    cpu = C.adam_ema_data(n)
    pad = cpu[6]
    st0 = torch.tensor(state, dtype=torch.float32)
    bufs = [t.clone() for t in base_n]
    st = st0.cuda()
    _groups_call(G, bufs, offset, n, ends, names, st)
    assert torch.equal(st.cpu(), st0) and _bits_equal(bufs[1], base_n[1])                  # state and gradient: untouched
    for buf, b0 in zip(bufs, base_n):                                                      # nothing outside [offset, offset + n)
        assert _bits_equal(buf[:offset], b0[:offset]) and _bits_equal(buf[offset + n:], b0[offset + n:])
    a = E.ema_weight(*EMA_CASE)
    lo = 0
    for hi, name in zip(ends, names):
        rng = slice(offset + lo, offset + hi)
        got = [b[rng] for b in bufs]
        if name in C.FROZEN:
            assert all(_bits_equal(x, b0[rng]) for x, b0 in zip(got, base_n)), (name, lo, hi)
        elif name == "default":
            plain = [t.clone() for t in base_n]
            _plain_call(G, plain, offset + lo, hi - lo, st0.cuda(), None, True)
            assert all(_bits_equal(x, q[rng]) for x, q in zip(got, plain)), (name, lo, hi)
            assert hi == lo or hi - lo < 3 or not _bits_equal(got[0], base_n[0][rng])
            # ... and to glowtts_adam_noam itself and glowtts_adam_noam_guarded (guard clear) on that range: p, m, v, no average
            for guard in (None, torch.zeros(4, device="cuda")):
                plain = [t.clone() for t in base_n]
                _plain_call(G, plain, offset + lo, hi - lo, st0.cuda(), guard, False)
                assert all(_bits_equal(x, q[rng]) for x, q in zip(got[:4], plain[:4])), (name, lo, hi, guard)
                assert _bits_equal(plain[4], base_n[4])
        else:
            p, g, m, v, e = (t[rng].cpu() for t in base_n)
            figs = C.figures(got[0], got[2], got[3], p, g, m, v, state, C.OPTIONS[name])
            fig_e = E.units(got[4], E.ema_ref(e, got[0].cpu(), a), e.double().abs() + got[0].cpu().double().abs())
            form = C.form_of(name)
            worst[form] = tuple(max(x, y) for x, y in zip(worst.get(form, (0.0,) * 4), figs + (fig_e,)))
            assert all(f <= b for f, b in zip(figs, C.BOUNDS[form])) and fig_e <= E.E_BOUND, (name, lo, hi, figs, fig_e, C.BOUNDS[form])
            if name == "scale0":                                               # live: the moments move, p stays bit for bit
                assert _bits_equal(got[0], base_n[0][rng])
                assert hi - lo < 3 or not _bits_equal(got[2], base_n[2][rng])
            # p = g = m = v = 0 (and e = 0): exactly zero afterwards — what keeps the padding of the flat buffers at zero
            z = pad[rng].cuda()
            assert all(bool((x[z] == 0).all()) for x in (got[0], got[2], got[3], got[4])), name
        lo = hi
    return bufs


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "off1"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"n{s[0]}-g{len(s[1])}-end{s[1][0]}")
def test_groups_update_raw(G, base, shape, offset):
    """glowtts_adam_noam_groups on [offset, offset + n) of buffers of n + 8 floats (offset 1: misaligned, the scalar form).
        n            ends                                  why
        5            5                                     one group
        5            2, 5                                  scalar form
        192          64, 128, 192                          three groups inside one wave's span of the vector form
        1023         1, 513, 1023                          scalar form, odd ends
        4224         64, 4160, 4224
        196          66, 128, 196                          aligned, n % 4 == 0, an end that is no multiple of 4: not the vector form
        2**21 + 192  2**20 + 64, 2**21 + 64, 2**21 + 192   one sweep of the 2048 x 256 x 4 grid is 2**21 floats: the last groups are
                                                           met in the grid-stride pass
        512          eight groups of 64                    the maximum
    Every layout of option sets (LAYOUTS: every set, frozen first, in the middle and last) with the average and guard = NULL is
    checked group by group (_check_layout); without the average p, m, v must be bit-equal to that run; with a cleared guard all
    four; a set guard leaves everything untouched.  The first layout also runs on the schedule's own rate (STATES[1])."""
    n, ends = shape
    base_n = base[n]
    layouts = LARGE_LAYOUTS if n > 2 ** 20 else LAYOUTS[len(ends)]
    worst = {}
    for i, names in enumerate(layouts):
        state = C.STATES[0]
        bufs = _check_layout(G, base_n, n, offset, ends, names, state, worst)
        st0 = torch.tensor(state, dtype=torch.float32)
        # ---- the form without the average: p, m, v as with it, e not touched
        bare = [t.clone() for t in base_n]
        _groups_call(G, bare, offset, n, ends, names, st0.cuda(), with_e=False)
        assert all(_bits_equal(bare[j], bufs[j]) for j in range(4)) and _bits_equal(bare[4], base_n[4]), names
        if i == 0:
            _check_layout(G, base_n, n, offset, ends, names, C.STATES[1], worst)
        # ---- the guarded forms, every layout (so a frozen range sits behind a guard at every shape): cleared = as without a
        # guard; set (any non-zero, NaN included) = nothing is touched
        for with_e in (True, False):
            for flag in (0.0, 1.0, NAN):
                held = [t.clone() for t in base_n]
                guard = torch.tensor([flag, 7.0, 8.0, 9.0], device="cuda")
                before = guard.clone()
                st = st0.cuda()
                _groups_call(G, held, offset, n, ends, names, st, guard=guard, with_e=with_e)
                want = (bufs if with_e else bare) if flag == 0.0 else base_n
                assert all(_bits_equal(x, y) for x, y in zip(held, want)), (names, with_e, flag)
                assert _bits_equal(guard, before) and torch.equal(st.cpu(), st0)
    for form, figs in sorted(worst.items()):
        print(f"groups n={n} ends={ends if len(ends) < 4 else '8 x 64'} offset={offset} {form}: m {figs[0]:.2f} u, v {figs[1]:.2f} u, "
              f"p {figs[2]:.2f} u (bounds {C.BOUNDS[form]}), e {figs[3]:.2f} u (bound {E.E_BOUND:g})")


def test_nine_groups_are_refused_and_nothing_is_written(G, base):
    n, ends = 576, tuple(64 * (k + 1) for k in range(9))
    bufs = [t.clone() for t in base[n]]
    st = torch.tensor(C.STATES[0], dtype=torch.float32).cuda()
    with pytest.raises(RuntimeError, match=r"n_groups = 9, expected 1 \.\. 8 \(GLOWTTS_MAX_PARAM_GROUPS\)"):
        _groups_call(G, bufs, 0, n, ends, ("l2",) * 9, st)
    torch.cuda.synchronize()
    assert all(_bits_equal(x, y) for x, y in zip(bufs, base[n]))


def test_bad_arguments_return_an_error_and_launch_nothing(G, base, monkeypatch):
    """Every refusal of include/glowtts_hip.h with real buffers behind the pointers: non-zero, its message, nothing written."""
    n, ends, names = 192, (64, 128, 192), ("l2", "decoupled", "scale0.1")
    bufs = [t.clone() for t in base[n]]
    st = torch.tensor(C.STATES[0], dtype=torch.float32).cuda()

    def refused(match, ends=ends, names=names, options=None, **kw):
        if options is not None:
            monkeypatch.setitem(C.OPTIONS, "bad", options)
            names = ("l2", "bad", "scale0.1")
        with pytest.raises(RuntimeError, match=match):
            _groups_call(G, bufs, 0, n, ends, names, st, **kw)

    refused("n_groups = 0", n_groups=0)
    refused("n_groups = -3", n_groups=-3)
    refused(r"ascend \(group 1\)", ends=(128, 64, 192))
    refused("end at n", ends=(64, 128, 191))
    refused("end at n", ends=(64, 128, 256))
    refused(r"lr_scale < 0 \(group 1\)", options=(-0.1, 0.0, 0, 0))
    refused("weight_decay < 0", options=(1.0, -0.01, 0, 0))
    for options in ((NAN, 0.0, 0, 0), (1.0, float("inf"), 0, 0), (1.0, 0.0, NAN, 0), (1.0, 0.0, 0, -float("inf"))):
        refused("non-finite option", options=options)
    for options in ((1.0, 0.0, 2, 0), (1.0, 0.0, 0, 0.5)):
        refused("must be 0 or 1", options=options)
    refused("ema_rate", case=(1.0, 0, 3))
    p, g, m, v, e = bufs
    end, opts = _tables(ends, names)
    tail = (C.LR, C.B1, C.B2, C.EPS, C.DIM, C.WARMUP, 0.1, 0, 1.0)
    for null_at in (0, 1, 2, 3, 6, 17, 18):
        args = [p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), e.data_ptr(), n, st.data_ptr(), None, *tail,
                ctypes.addressof(end), ctypes.addressof(opts), 3]
        args[null_at] = None
        with pytest.raises(RuntimeError, match="glowtts_adam_noam_groups: null pointer"):
            G.hip.call("glowtts_adam_noam_groups", *args)
    torch.cuda.synchronize()
    assert all(_bits_equal(x, y) for x, y in zip(bufs, base[n]))
    assert torch.equal(st.cpu(), torch.tensor(C.STATES[0], dtype=torch.float32))


# =============================================================================================== 2. the optimizer
SIZES = (1, 65, 4099)
GROUPS = ({}, {"lr_scale": 0.1, "weight_decay": 1e-2}, {"weight_decay": 1e-2, "decoupled_weight_decay": True})
SCALES = (1.0, 0.1, 1.0)
DIM, WARM = 192, 10
HYPER = (C.f32(0.9), C.f32(0.98), C.f32(1e-9))


def _noam(k, lr):
    return lr * DIM ** -0.5 * min(k ** -0.5, k * WARM ** -1.5)


def _optimizer(G, init, options, scheduler="noam", lr=1.0, **kw):
    params = [torch.nn.Parameter(t.clone().cuda()) for t in init]
    groups = params if options is None else [{"params": [p], **o} for p, o in zip(params, options)]
    opt = G.optimize.Adam(groups, scheduler=scheduler, dim_model=DIM, warmup_steps=WARM, lr=lr, betas=HYPER[:2], eps=HYPER[2], **kw)
    return params, opt


def _grads(gen, sizes):
    out = []
    for n in sizes:
        g = torch.randn(n, generator=gen)
        out.append(torch.where(g >= 0, g + 1e-3, g - 1e-3))                  # |g| >= 1e-3
    return out


def _padding(flat):
    pad = torch.ones(flat.numel_padded, dtype=torch.bool)
    for o, n in flat.slices():
        pad[o: o + n] = False
    return pad.cuda()


def _trajectory(G, scheduler, updates, lr, seed):
    """`updates` updates of three parameters of 1, 65 and 4099 elements in the groups GROUPS through optimize.Adam against
    torch.optim.Adam on fp64 CPU copies with the same groups, whose group rates are set to rate(k) * lr_scale before update k.
    e_ref — the same run by torch in fp32 on the CPU against the fp64 run — sets the bound: per tensor max|p - p64| <=
    max(4 e_ref, 16 u max|p|).  The host mirror: param_groups[k]["lr"] == cur_lr * lr_scale after every step and after
    sync_from_device()."""
    gen = torch.Generator().manual_seed(seed)
    init = [torch.randn(n, generator=gen) for n in SIZES]
    params, opt = _optimizer(G, init, GROUPS, scheduler, lr)
    flat = opt._optim
    pad = _padding(flat)

    def torch_ref(dtype):
        ps = [t.to(dtype).requires_grad_(True) for t in init]
        groups = [{"params": [p], **{k: v for k, v in o.items() if k != "lr_scale"}} for p, o in zip(ps, GROUPS)]
        return ps, torch.optim.Adam(groups, lr=lr, betas=HYPER[:2], eps=HYPER[2])

    p64, ref64 = torch_ref(torch.float64)
    p32, ref32 = torch_ref(torch.float32)

    def mirror_ok():
        return [g["lr"] for g in flat.param_groups] == [opt.cur_lr * s for s in SCALES]

    mirrors = [mirror_ok()]                                                  # (asserted last: the parameters say more when both fail)
    for k in range(1, updates + 1):
        rate = _noam(k, lr) if scheduler == "noam" else lr
        assert abs(opt.cur_lr - rate) <= 1e-12 * rate
        for ref in (ref64, ref32):
            for group, scale in zip(ref.param_groups, SCALES):
                group["lr"] = rate * C.f32(scale)
        for i, g in enumerate(_grads(gen, SIZES)):
            params[i].grad.copy_(g)
            p64[i].grad, p32[i].grad = g.double(), g.clone()
        opt.step()
        ref64.step()
        ref32.step()
        mirrors.append(mirror_ok())
        for buf in (flat.flat_p, flat.flat_m, flat.flat_v):
            assert bool((buf[pad] == 0).all()), k
    assert opt.sync_from_device() == {"applied": 0, "skipped": 0, "consecutive_skipped": 0}
    mirrors.append(mirror_ok())
    assert float(flat.dev_state[0]) == updates + 1
    for i, n in enumerate(SIZES):
        want = p64[i].detach()
        e_ref = float((p32[i].detach().double() - want).abs().max())
        err = float((params[i].detach().cpu().double() - want).abs().max())
        bound = max(4 * e_ref, 16 * C.U * float(want.abs().max()))
        print(f"grouped trajectory scheduler={scheduler} {updates} updates, group {i} {GROUPS[i]} ({n} elements): max|p - p64| = "
              f"{err:.3e}, fp32 CPU torch e_ref = {e_ref:.3e}, bound {bound:.3e}")
        assert err <= bound, (n, GROUPS[i], err, e_ref, bound)
    assert all(mirrors), mirrors


def test_grouped_trajectory_noam_vs_torch_fp64(G):
    """Fails without the feature: the decay groups come out as plain Adam."""
    _trajectory(G, "noam", 30, 1.0, seed=21)


def test_grouped_trajectory_constant_rate_vs_torch_fp64(G):
    _trajectory(G, None, 5, C.f32(0.01), seed=22)


def test_a_frozen_group_is_left_alone_and_its_average_stays_its_parameters(G):
    """A fourth, frozen group beside the three of the trajectory, with ema_decay: after 3 updates its parameters and (non-zero)
    moments are bit-equal, its slice of flat_e equals its slice of flat_p, the live groups moved, all padding stays zero."""
    gen = torch.Generator().manual_seed(23)
    sizes = SIZES + (130,)
    init = [torch.randn(n, generator=gen) for n in sizes]
    params, opt = _optimizer(G, init, GROUPS + ({"frozen": True, "weight_decay": 0.5},), ema_decay=0.9)
    flat = opt._optim
    pad = _padding(flat)
    o, n = flat.slices()[3]
    assert flat.group_ends[2] == o and flat.group_ends[3] == flat.numel_padded
    flat.flat_m[o:o + n].normal_(generator=None)
    flat.flat_v[o:o + n].uniform_()
    before = [b.clone() for b in (flat.flat_p, flat.flat_m, flat.flat_v)]
    for _ in range(3):
        for p, g in zip(params, _grads(gen, sizes)):
            p.grad.copy_(g)
        opt.step()
    for b0, b in zip(before, (flat.flat_p, flat.flat_m, flat.flat_v)):
        assert _bits_equal(b[o:], b0[o:]) and not _bits_equal(b[:o], b0[:o])
    assert _bits_equal(params[3].detach(), init[3].cuda())
    assert _bits_equal(flat.flat_e[o:], flat.flat_p[o:]) and not _bits_equal(flat.flat_e[:o], flat.flat_p[:o])
    for buf in (flat.flat_p, flat.flat_m, flat.flat_v, flat.flat_e):
        assert bool((buf[pad] == 0).all())
    assert opt.ema_num_updates() == 3


@pytest.mark.parametrize("options", [({},), ({}, {}, {})], ids=["one-default-group", "three-default-groups"])
@pytest.mark.parametrize("form", [{}, {"skip_nonfinite": True}, {"ema_decay": 0.99}], ids=["plain", "guarded", "ema"])
def test_default_groups_launch_what_they_launched_before(G, monkeypatch, options, form):
    """Groups at defaults: `step()` calls today's entry points, never the grouped one, and the result is bit-equal to an optimizer
    built from a plain parameter list."""
    gen = torch.Generator().manual_seed(24)
    sizes = SIZES if len(options) == 3 else SIZES[2:]
    init = [torch.randn(n, generator=gen) for n in sizes]
    plain_params, plain = _optimizer(G, init, None, **form)
    params, opt = _optimizer(G, init, options, **form)
    assert len(opt._optim.param_groups) == len(options) and opt._optim.offsets == plain._optim.offsets
    names = []
    real = G.optimize.call
    monkeypatch.setattr(G.optimize, "call", lambda name, *a, **k: (names.append(name), real(name, *a, **k))[1])
    for _ in range(2):
        grads = _grads(gen, sizes)
        for ps, o in ((plain_params, plain), (params, opt)):
            for p, g in zip(ps, grads):
                p.grad.copy_(g)
            names.clear()
            o.step()
            update = "glowtts_adam_noam_ema" if "ema_decay" in form else "glowtts_adam_noam" + ("_guarded" if form else "")
            assert names == [update, "glowtts_adam_advance" + ("_guarded" if "skip_nonfinite" in form else "")], names
    for a, b in ((opt._optim.flat_p, plain._optim.flat_p), (opt._optim.flat_m, plain._optim.flat_m),
                 (opt._optim.flat_v, plain._optim.flat_v)):
        assert _bits_equal(a, b)
    # one non-default option and the grouped entry takes the update's place; the advance call stays
    opt._optim.param_groups[-1]["weight_decay"] = 1e-2
    names.clear()
    opt.step()
    assert names == ["glowtts_adam_noam_groups", "glowtts_adam_advance" + ("_guarded" if "skip_nonfinite" in form else "")]


def test_a_nan_in_a_frozen_groups_gradient_still_skips_the_update(G):
    """The clip pass does not know groups: its non-finite test covers the frozen range.  guard counters as in
    tests/test_update_guard.py: [0, 1, 1, 0] after the skipped update, [0, 1, 0, 1] after the clean one that follows."""
    gen = torch.Generator().manual_seed(25)
    sizes = SIZES + (130,)
    init = [torch.randn(n, generator=gen) for n in sizes]
    params, opt = _optimizer(G, init, GROUPS + ({"frozen": True},), skip_nonfinite=True)
    flat = opt._optim
    for p, g in zip(params, _grads(gen, sizes)):
        p.grad.copy_(g)
    params[3].grad[7] = NAN
    before = [b.clone() for b in (flat.flat_p, flat.flat_m, flat.flat_v, flat.dev_state)]
    assert flat.clip_grad_value_(CLIP) is not None
    opt.step()
    assert flat.guard.tolist() == [0.0, 1.0, 1.0, 0.0]
    assert all(_bits_equal(a, b) for a, b in zip((flat.flat_p, flat.flat_m, flat.flat_v, flat.dev_state), before))
    assert opt.sync_from_device() == {"applied": 0, "skipped": 1, "consecutive_skipped": 1}
    for p, g in zip(params, _grads(gen, sizes)):
        p.grad.copy_(g)
    flat.clip_grad_value_(CLIP)
    opt.step()
    assert flat.guard.tolist() == [0.0, 1.0, 0.0, 1.0]
    o = flat.slices()[3][0]
    assert _bits_equal(flat.flat_p[o:], before[0][o:]) and not _bits_equal(flat.flat_p[:o], before[0][:o])


class _Holder(torch.nn.Module):
    def __init__(self, params):
        super().__init__()
        self.ps = torch.nn.ParameterList(params)


def test_checkpoint_round_trip_continues_bit_for_bit(G, tmp_path):
    """Four updates, save through checkpoint.save_checkpoint, load into a FRESH three-group optimizer, a fifth update on both:
    parameters and moments bit-equal to the uninterrupted run's."""
    gen = torch.Generator().manual_seed(26)
    init = [torch.randn(n, generator=gen) for n in SIZES]
    params, opt = _optimizer(G, init, GROUPS)
    for _ in range(4):
        for p, g in zip(params, _grads(gen, SIZES)):
            p.grad.copy_(g)
        opt.step()
    path = tmp_path / "groups.pth"
    G.checkpoint.save_checkpoint(G.checkpoint.Checkpoint(model=_Holder(params), optimizer=opt, learning_rate=opt.cur_lr,
                                                         global_step=5, version=1), path)
    file = torch.load(path, map_location="cpu", weights_only=True)
    assert [g["params"] for g in file["optimizer"]["param_groups"]] == [[0], [1], [2]]
    assert [(g["lr_scale"], g["weight_decay"], g["decoupled_weight_decay"]) for g in file["optimizer"]["param_groups"]] == [
        (1.0, 0, False), (0.1, 1e-2, False), (1.0, 1e-2, True)]
    params2, opt2 = _optimizer(G, [torch.zeros(n) for n in SIZES], ({}, {}, {}))
    back = G.checkpoint.load_checkpoint(path, None, model=_Holder(params2), optimizer=opt2)
    assert back.global_step == 5 and opt2._optim._group_options() == opt._optim._group_options()
    assert _bits_equal(opt2._optim.flat_p, opt._optim.flat_p) and _bits_equal(opt2._optim.flat_m, opt._optim.flat_m)
    grads = _grads(gen, SIZES)
    for ps, o in ((params, opt), (params2, opt2)):
        for p, g in zip(ps, grads):
            p.grad.copy_(g)
        o.step()
    fa, fb = opt._optim, opt2._optim
    assert _bits_equal(fa.flat_p, fb.flat_p) and _bits_equal(fa.flat_m, fb.flat_m) and _bits_equal(fa.flat_v, fb.flat_v)
    assert float(fb.dev_state[0]) == 6.0 and float(fb.dev_state[3]) == 0.0


# =============================================================================================== 3. one training step
@pytest.fixture(scope="module")
def small():
    """The small multi-speaker config of tests/test_grad_accum.py (hidden 64, 3 blocks, 2 WN layers, dropout 0), B = 2, T_mel = 64."""
    from oracle import glow_oracle as O

    hp = O.HParams(n_vocab=60, hidden_channels=64, filter_channels=128, filter_channels_dp=64, n_layers_enc=2,
                   n_blocks_dec=3, n_block_layers=2, n_speakers=4, gin_channels=16, mean_only=False)
    sd = O.init_state_dict(hp, seed=5)
    gen = torch.Generator().manual_seed(1)
    for k in list(sd):
        if k.endswith(".end.weight"):
            sd[k] = 0.05 * torch.randn(sd[k].shape, generator=gen)
    xl, yl = torch.tensor([12, 7]), torch.tensor([64, 33])
    x = torch.randint(1, 60, (2, 12), generator=gen) * (torch.arange(12)[None] < xl[:, None])
    y = torch.randn(2, 80, 64, generator=gen) * (torch.arange(64)[None, None] < yl[:, None, None])
    batch = tuple(t.cuda() for t in (x, xl, y, yl, torch.tensor([1, 2])))
    return types.SimpleNamespace(hp=hp, sd=sd, batch=batch)


def _small_model(G, small):
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
    return m.cuda().train()


def test_a_step_with_a_frozen_encoder(G, small):
    """named_param_groups(model, {"encoder.": frozen, "decoder.": lr_scale 0.5}), one train_batch: every encoder.* parameter is
    bit-equal afterwards, every decoder.* parameter (and the default group's emb_g) moved, the loss is finite, every gradient is
    still a view of flat_g (so the native path saw nothing of the freeze), and FlowBlockReducer accepts the layout.

    "Moved" is asserted as `moved == the parameter's gradient has a non-zero element`, for every parameter outside the encoder, and
    at least 90 % of them must have moved.  The only exemption is a parameter whose whole gradient is exactly zero in this one
    step (one the loss of this small configuration does not depend on): from zero
    moments, m' = (1 - b1) g = 0 and v' = 0, so the update is 0 / (0 + eps) = 0 and Adam cannot move it, with or without groups.
    The assertion's failure message names every parameter for which the two differ."""
    model = _small_model(G, small)
    groups = G.optimize.named_param_groups(model, {"encoder.": {"frozen": True}, "decoder.": {"lr_scale": 0.5}})
    assert [{k: v for k, v in g.items() if k != "params"} for g in groups] == [{"frozen": True}, {"lr_scale": 0.5}, {}]
    opt = G.optimize.Adam(groups, scheduler="noam", dim_model=64, warmup_steps=10, lr=1.0)     # (first rate 4e-3: every step shows in fp32)
    flat = opt._optim
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    assert all(p.requires_grad for p in model.parameters())
    loss = G.train.train_batch(model, opt, small.batch, CLIP)
    assert bool(torch.isfinite(loss))
    assert flat.grads_in_place()
    lo, hi = flat.flat_g.data_ptr(), flat.flat_g.data_ptr() + 4 * flat.numel_padded
    moved, with_grad = {}, {}
    for name, p in model.named_parameters():
        assert lo <= p.grad.data_ptr() and p.grad.data_ptr() + 4 * p.numel() <= hi, name
        moved[name] = not _bits_equal(p.detach(), before[name])
        with_grad[name] = bool((p.grad != 0).any())                          # (the clipped gradient is still in flat_g)
    encoder = [k for k in moved if k.startswith("encoder.")]
    others = [k for k in moved if not k.startswith("encoder.")]
    assert not any(moved[k] for k in encoder)
    assert sum(with_grad[k] for k in encoder) >= 0.9 * len(encoder)          # they HAVE gradients: only the update leaves them alone
    assert all(moved[k] == with_grad[k] for k in others), [k for k in others if moved[k] != with_grad[k]]
    assert sum(moved[k] for k in others) >= 0.9 * len(others) and any(k.startswith("decoder.") for k in others)
    # the groups are contiguous in model order: the data-parallel reducer builds (no process group: one rank)
    red = G.parallel.FlowBlockReducer(model, opt)
    assert len(red.buckets) >= 1 and red.buckets[-1].hi <= flat.numel_padded
    first_decoder = next(o for (o, _), (n, _) in zip(flat.slices(), model.named_parameters()) if n.startswith("decoder."))
    assert flat.group_ends[0] == first_decoder and flat.group_ends[-1] == flat.numel_padded
