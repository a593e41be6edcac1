"""The backward of a WN stack as csrc/wn_stack.hip queues it: the decision (csrc/wn_plan.hpp, glowtts_wn_bwd_plan_for) on the CPU, and
every form of the launch sequence on the GPU against the per-operator Python path.

1. The plan, no device.  glowtts_wn_bwd_plan_for over n_layers 1..10 x H {48, 64, 96, 192, 384} x T {0, 4, 6, 8, 12} x dilation rate
   {1, 2} x tensor type {fp32, bf16} x {glowtts_wn_bwd, glowtts_flow_block_bwd} x every value of two_source the callers use x WRW_BATCH
   {0, 1}: every field against `_parent_rules`, which restates the rules as wn_stack.hip and convops.py spelled them BEFORE the plan
   existed (one copy per place then; the expressions are copied from there, not from the new header), the rejections, and the d_rs
   element count against what the three autograd nodes used to allocate.

2. The launch sequences, on the GPU (rows A .. F of ROWS / the stand-alone tests).  Only entry points and switches that predate the
   plan are used, so this part also runs against a tree without it.  A row is a FlowSpecDecoder of two blocks (batch 2, 24 mel
   frames = 12 after the squeeze: T % 4 == 0 and shorter than any frame tile; lengths 24 and 14, so per-utterance strides matter) or
   the bare WN module, inside `_hip.zero_scope` — a training step, the weight-gradient stream in use — compared with the same module
   driven operator by operator from Python (convops._WN_NATIVE = "off"), at the tolerances tests/test_hip_parity.py uses for exactly
   this comparison.  Rows that differ only in WHEN the weight gradients are queued run the same chain kernels in the same order:
   their dx and z are equal bit for bit.
"""
import ctypes
import functools
import itertools

import pytest
import torch

from helpers import assert_close


# ================================================================================================ 1. the plan, no device
AFTER_CHAIN, BATCHED, PER_LAYER = 0, 1, 2
FIELDS = ("two_source_ok", "two_source", "pre_masked", "block_wrw1", "wrw_order", "chain_calls", "wgrad_calls", "d_rs_elems")
GRID = list(itertools.product(range(1, 11), (48, 64, 96, 192, 384), (0, 4, 6, 8, 12), (1, 2), (0, 1)))
B, TAPS = 3, 5


def _parent_rules(n, H, T, dil_rate, io, two_source, in_block, wrw_batch):
    """None where the executor rejected the call, else the plan's fields in the order of FIELDS."""
    if in_block:                                         # glowtts_flow_block_bwd_io
        if io and two_source:                            # "bf16 tensors use the d_rs form"
            return None
        multi1 = bool(two_source) and not io and n >= 1 and n + 2 <= 8 and H % 64 == 0
        pre_mask = 1 if (two_source and not io) else 0
        two_source = (1 | (pre_mask << 1) | (4 if (multi1 and pre_mask) else 0)) if two_source else 0
    elif io and two_source:                              # glowtts_wn_bwd_io: "bf16 tensors use the d_rs form with a masked input gradient"
        return None
    pre_masked = (two_source & 2) != 0
    skip_wrw1 = (two_source & 4) != 0 and pre_masked
    two_source &= 1
    ok = (not io) and dil_rate == 1 and H % 192 == 0 and T % 4 == 0          # convops._two_src
    if not two_source:
        # the chain: res_skip_bwd, conv_gate_bwd, conv_fwd per layer; then wrw_any twice per layer
        return (int(ok), 0, 0, 0, AFTER_CHAIN, 3 * n, 2 * n, n * B * 2 * H * T)
    if not (dil_rate == 1 and H % 192 == 0 and T % 4 == 0):                  # "two-source form needs dilation 1, ..."
        return None
    chain = 2 * n + (0 if pre_masked else 1)             # conv_gate_bwd, conv_fwd per layer; res_skip_bwd of the last layer
    if wrw_batch and n <= 8:
        wgrad = 1 + (0 if skip_wrw1 else 1 + (1 if n > 1 else 0))            # wrw_batch (5 taps); conv_wrw (last), wrw_batch (1x1)
        order = BATCHED
    else:
        wgrad = n + (0 if skip_wrw1 else n)              # conv_wrw (5 taps) per layer; conv_wrw / conv_wrw2 per layer
        order = PER_LAYER
    return (1, 1, int(pre_masked), int(skip_wrw1), order, chain, wgrad, B * H * T)


@pytest.fixture
def wrw_batch_knob():
    """Sets the library's WRW_BATCH switch; the value found is put back afterwards."""
    from glow_tts_train import _hip

    before = _hip.get_knob("WRW_BATCH")
    yield lambda v: _hip.set_knob("WRW_BATCH", v)
    _hip.set_knob("WRW_BATCH", before)


@pytest.mark.parametrize("wrw_batch", [1, 0])
def test_plan_matches_the_rules_it_replaced(wrw_batch, wrw_batch_knob):
    from glow_tts_train import _hip

    lib = _hip.load()
    wrw_batch_knob(wrw_batch)
    out = _hip.WnBwdPlan()
    ref, fn = ctypes.byref(out), lib.glowtts_wn_bwd_plan_for
    forms = {}
    for (n, H, T, dil, io), (in_block, two_source) in itertools.product(GRID, [(0, 0), (0, 1), (0, 3), (0, 7), (0, 2), (0, 5), (0, 6),
                                                                            (0, 9), (1, 0), (1, 1)]):
        want = _parent_rules(n, H, T, dil, io, two_source, in_block, wrw_batch)
        rc = fn(n, B, H, T, TAPS, dil, io, two_source, in_block, ref)
        what = f"n={n} H={H} T={T} dil={dil} io={io} two_source={two_source} in_block={in_block} WRW_BATCH={wrw_batch}"
        if want is None:
            assert rc != 0 and lib.glowtts_last_error().decode().startswith("glowtts_wn_bwd_plan_for: "), what
            continue
        assert rc == 0, what + ": " + lib.glowtts_last_error().decode()
        got = tuple(int(getattr(out, f)) for f in FIELDS)
        assert got == want, f"{what}: {dict(zip(FIELDS, got))} != {dict(zip(FIELDS, want))}"
        forms[got[1:5]] = forms.get(got[1:5], 0) + 1
    # the grid reaches every form: d_rs; two-source x {un-masked, pre-masked, 1x1s the block's} in this switch's orders
    orders = (BATCHED, PER_LAYER) if wrw_batch else (PER_LAYER,)
    assert set(forms) == {(0, 0, 0, AFTER_CHAIN)} | {(1, pm, b1, o) for o in orders for pm, b1 in ((0, 0), (1, 0), (1, 1))}, forms


def test_plan_rejections():
    from glow_tts_train import _hip

    lib = _hip.load()
    out = _hip.WnBwdPlan()
    ref, fn = ctypes.byref(out), lib.glowtts_wn_bwd_plan_for
    for args, match in [((0, 2, 192, 12, 5, 1, 0, 0, 0), "bad shape"), ((2, -1, 192, 12, 5, 1, 0, 0, 0), "bad shape"),
                        ((2, 2, 0, 12, 5, 1, 0, 0, 0), "bad shape"), ((2, 2, 192, -4, 5, 1, 0, 0, 0), "bad shape"),
                        ((2, 2, 192, 12, 4, 1, 0, 0, 0), "bad shape"), ((2, 2, 192, 12, 0, 1, 0, 0, 0), "bad shape"),
                        ((2, 2, 192, 12, 5, 0, 0, 0, 0), "bad shape"), ((2, 2, 192, 12, 5, 1, 1, 1, 0), "bf16 tensors"),
                        ((2, 2, 192, 12, 5, 1, 1, 2, 0), "bf16 tensors"), ((2, 2, 192, 12, 5, 1, 1, 1, 1), "bf16 tensors"),
                        ((2, 2, 48, 12, 5, 1, 0, 1, 0), "two-source form needs"), ((2, 2, 192, 6, 5, 1, 0, 1, 1), "two-source form needs"),
                        ((2, 2, 192, 12, 5, 2, 0, 3, 0), "two-source form needs")]:
        assert fn(*args, ref) != 0, args
        msg = lib.glowtts_last_error().decode()
        assert msg.startswith("glowtts_wn_bwd_plan_for: ") and match in msg, (args, msg)
    assert fn(2, 2, 192, 12, 5, 1, 0, 1, 0, None) != 0
    assert lib.glowtts_last_error().decode().startswith("glowtts_wn_bwd_plan_for: ")
    assert fn(2, 0, 192, 0, 5, 1, 0, 1, 1, ref) == 0 and out.d_rs_elems == 0          # an empty batch is planned, not refused


def test_d_rs_size_is_what_the_nodes_allocated():
    """convops._wn_bwd_plan (the form, the element count) against the expressions FlowBlockFn / FlowStackFn (`_two_src`) and
    WNFn._backward_native (`wgrad.enabled and ...`) carried themselves: d_rs (B, H, T) or (n_layers, B, 2H, T)."""
    from glow_tts_train import convops

    for (n, H, T, dil, io), in_block, enabled in itertools.product(GRID, (True, False), (True, False)):
        if in_block:
            two_src = (not io) and dil == 1 and H % 192 == 0 and T % 4 == 0
            got = convops._wn_bwd_plan(n, B, H, T, TAPS, dil, io, True)
        elif io:
            continue                                     # the stand-alone node has fp32 tensors only
        else:
            two_src = enabled and dil == 1 and H % 192 == 0 and T % 4 == 0
            got = convops._wn_bwd_plan(n, B, H, T, TAPS, dil, 0, False, want=enabled)
        want = torch.Size((B, H, T) if two_src else (n, B, 2 * H, T)).numel()
        assert got == (bool(two_src), want), (n, H, T, dil, io, in_block, enabled, got)


# ================================================================================================ 2. the launch sequences, on the GPU
def _traced(convops, names):
    """convops.call wrapped: the argument lists of the calls to `names` are kept.  -> (the list, undo)"""
    seen, orig = [], convops.call

    def call(name, *args, **kw):
        if name in names:
            seen.append((name, args))
        return orig(name, *args, **kw)
    convops.call = call
    return seen, lambda: setattr(convops, "call", orig)


@functools.lru_cache(maxsize=None)
def _decoder_run(h, n_layers, mode, wrw_batch):
    """One training step of a two-block decoder.  mode: "stack" (every block in one autograd node), "block" (a node per block),
    "off" (the per-operator path: the reference).  -> (z, logdet, dx, parameter gradients, two_source of each block's backward call)"""
    from glow_tts_train import _hip, convops, models

    torch.manual_seed(77)
    dec = models.FlowSpecDecoder(80, h, kernel_size=5, dilation_rate=1, n_blocks=2, n_layers=n_layers, p_dropout=0.05, n_split=4,
                                 n_sqz=2).cuda().train()
    with torch.no_grad():
        for f in dec.flows:
            if hasattr(f, "end"):
                f.end.weight.normal_(0, 0.02)
            if hasattr(f, "logs"):
                f.logs.normal_(0, 0.1)
                f.bias.normal_(0, 0.1)
    b, t = 2, 24
    y0 = torch.randn(b, 80, t, device="cuda")
    lens = torch.tensor([24, 14], device="cuda")
    mask = (torch.arange(t, device="cuda")[None] < lens[:, None]).float().unsqueeze(1)
    r, s = torch.randn(b, 80, t, device="cuda"), torch.randn(b, device="cuda")
    for p in dec.parameters():
        p.grad = torch.zeros_like(p)
    knob, native, stack = _hip.get_knob("WRW_BATCH"), convops._WN_NATIVE, models._FLOW_STACK
    seen, undo = _traced(convops, ("glowtts_flow_block_bwd_io",))
    try:
        _hip.set_knob("WRW_BATCH", wrw_batch)
        convops._WN_NATIVE = "off" if mode == "off" else "both"
        models._FLOW_STACK = mode == "stack"
        torch.manual_seed(5)                             # the same keep-masks in every run
        with _hip.zero_scope(y0.device):
            y = (y0 * mask).clone().requires_grad_(True)
            z, ld = dec(y, mask)
            ((z * r).sum() + (ld * s).sum()).backward()
            _hip.join_side_streams()
            convops.flush_groups()
        torch.cuda.synchronize()
    finally:
        undo()
        convops._WN_NATIVE, models._FLOW_STACK = native, stack
        _hip.set_knob("WRW_BATCH", knob)
    grads = {k: p.grad.clone() for k, p in dec.named_parameters()}
    return z.detach().clone(), ld.detach().clone(), y.grad.clone(), grads, tuple(a[-3] for _, a in seen)


@functools.lru_cache(maxsize=None)
def _wn_run(mode, wrw_batch, scope):
    """One forward + backward of the bare WN module (two layers), inside `zero_scope` (the weight-gradient stream in use) or not.
    -> (y, dx, parameter gradients, two_source of the glowtts_wn_bwd call)"""
    from glow_tts_train import _hip, convops, layers

    torch.manual_seed(31)
    wn = layers.WN(160, 192, kernel_size=5, dilation_rate=1, n_layers=2, p_dropout=0.05).cuda().train()
    b, t = 2, 12
    x0 = torch.randn(b, 192, t, device="cuda")
    lens = torch.tensor([12, 7], device="cuda")
    mask = (torch.arange(t, device="cuda")[None] < lens[:, None]).float()[:, None]
    r = torch.randn(b, 192, t, device="cuda")
    for p in wn.parameters():
        p.grad = torch.zeros_like(p)
    knob, native = _hip.get_knob("WRW_BATCH"), convops._WN_NATIVE
    seen, undo = _traced(convops, ("glowtts_wn_bwd",))

    def step():
        x = (x0 * mask).clone().requires_grad_(True)
        y = wn(x, mask)
        (y * r).sum().backward()
        return x, y
    try:
        _hip.set_knob("WRW_BATCH", wrw_batch)
        convops._WN_NATIVE = mode
        torch.manual_seed(77)                            # the same keep-masks in every run
        if scope:
            with _hip.zero_scope(x0.device):
                x, y = step()
                _hip.join_side_streams()
        else:
            x, y = step()
        torch.cuda.synchronize()
    finally:
        undo()
        convops._WN_NATIVE = native
        _hip.set_knob("WRW_BATCH", knob)
    return y.detach().clone(), x.grad.clone(), {k: p.grad.clone() for k, p in wn.named_parameters()}, tuple(a[-2] for _, a in seen)


def _check(what, got, want):
    """(output, [logdet,] dx, gradients) against the per-operator path's."""
    assert_close(got[0], want[0], what=f"{what}: y", rtol=1e-6, atol=1e-6)
    if len(got) == 4:
        assert_close(got[1], want[1], what=f"{what}: logdet", rtol=1e-6, atol=1e-4)
    dx, dx0 = got[-2], want[-2]
    assert_close(dx, dx0, what=f"{what}: dx", rtol=1e-5, atol=1e-6 * float(dx0.abs().max()))
    assert sorted(got[-1]) == sorted(want[-1])
    for k, g0 in want[-1].items():
        assert_close(got[-1][k], g0, what=f"{what}: grad {k}", rtol=2e-4, atol=2e-5 * max(1.0, float(g0.abs().max())))


# row: (hidden width, n_layers, caller, WRW_BATCH, two_source the block's backward is called with) and what it reaches
ROWS = {
    "A-stack": (192, 2, "stack", 1, 1),     # two-source, pre-masked, the 1x1 weight gradients in the block's one launch
    "A-block": (192, 2, "block", 1, 1),     # ... from the per-block node
    "B": (192, 7, "stack", 1, 1),           # batched order with the stack's own 1x1 launches (7 + 2 problems do not fit the block's table)
    "C": (192, 9, "stack", 1, 1),           # per-layer order: 9 layers do not fit the batch tables
    "D": (192, 2, "stack", 0, 1),           # per-layer order by the switch, the 1x1 weight gradients still the block's
    "F-block": (48, 2, "stack", 1, 0),      # the d_rs form: H % 192 != 0
}


@pytest.mark.gpu
@pytest.mark.parametrize("row", sorted(ROWS))
def test_block_backward_forms_match_per_op_path(row):
    h, n_layers, mode, wrw_batch, two_source = ROWS[row]
    *got, flags = _decoder_run(h, n_layers, mode, wrw_batch)
    *want, flags_off = _decoder_run(h, n_layers, "off", 1)
    assert flags == (two_source, two_source) and flags_off == (), (flags, flags_off)      # both blocks through the executor / none
    _check(row, got, want)


@pytest.mark.gpu
def test_block_weight_gradient_order_leaves_the_chain_alone():
    """A against D: WRW_BATCH moves the weight gradients, the chain's kernels and their order stay: z and dx bit for bit."""
    a, d = _decoder_run(192, 2, "stack", 1), _decoder_run(192, 2, "stack", 0)
    assert torch.equal(a[0], d[0]) and torch.equal(a[2], d[2])


@pytest.mark.gpu
@pytest.mark.parametrize("wrw_batch", [1, 0])
def test_wn_alone_two_source_unmasked_matches_layer_by_layer_path(wrw_batch):
    """Row E: glowtts_wn_bwd's two-source form with a dskip that is NOT masked yet (the last layer's res_skip_bwd launch), which
    needs the weight-gradient stream: batched and per-layer order."""
    *got, flags = _wn_run("both", wrw_batch, True)
    *want, flags_off = _wn_run("off", 1, True)
    assert flags == (1,) and flags_off == (), (flags, flags_off)
    _check(f"E WRW_BATCH={wrw_batch}", got, want)


@pytest.mark.gpu
def test_wn_alone_weight_gradient_order_leaves_the_chain_alone():
    e1, e0 = _wn_run("both", 1, True), _wn_run("both", 0, True)
    assert torch.equal(e1[0], e0[0]) and torch.equal(e1[1], e0[1])


@pytest.mark.gpu
def test_wn_alone_d_rs_form_matches_layer_by_layer_path():
    """Row F: outside a training step the weight gradients stay on the one stream and glowtts_wn_bwd is asked for the d_rs form."""
    *got, flags = _wn_run("both", 1, False)
    *want, flags_off = _wn_run("off", 1, False)
    assert flags == (0,) and flags_off == (), (flags, flags_off)
    _check("F WN alone", got, want)
