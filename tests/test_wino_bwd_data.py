"""The backward-data of the WN stack's gated 5-tap in-conv in Winograd F(4, 5) form (csrc/convwino.hip, wino_bwd_kernel):
dx = (W_in^T (*) d_xin [+ addend]) [* mask] with the in-conv's packed backward weights (M = H = 192 rows, 2H input channels),
the two halves of the input channels computed by two workgroups and combined inside the launch by the one that finishes last."""
import sys

import pytest
import torch
import torch.nn.functional as F

H = 192


@pytest.fixture
def M():
    from glow_tts_train import _hip, convops

    _hip.load()

    class NS:
        pass

    ns = NS()
    ns.hip, ns.convops = _hip, convops
    before = convops.conv_math_name()
    yield ns
    _hip.conv_bind_planes(None)
    _hip.conv_bind_wino(None)
    _hip.set_knob("WINO_BWD", 1)
    convops.set_conv_math(before)


def _problem(b, t, seed, h=H):
    dev = "cuda"
    torch.manual_seed(seed)
    d_xin = torch.randn(b, 2 * h, t, device=dev) * torch.exp(torch.randn(1, 2 * h, 1, device=dev) * 0.5)
    v_in = torch.randn(2 * h, h, 5, device=dev) * 0.03
    lens = torch.randint(max(1, t // 2), t + 1, (b,), device=dev)
    lens[0] = t
    mask = (torch.arange(t, device=dev)[None] < lens[:, None]).float()
    addend = torch.randn(b, h, t, device=dev)
    return d_xin, v_in, mask, addend


class _Bound:
    """The in-conv's backward pack alone as the packed buffer: its bf16 planes and its U planes bound to this thread."""

    def __init__(self, M, wp_b, h=H):
        self.M, self.wp_b = M, wp_b
        call, ptr = M.hip.call, M.hip.ptr
        self.planes = torch.empty(3 * wp_b.numel(), device=wp_b.device, dtype=torch.int16)
        call("glowtts_conv_split_weights", ptr(wp_b), wp_b.numel(), ptr(self.planes))
        n_u = M.hip.wino_plane_elems(wp_b.numel())
        self.u = torch.zeros(3 * n_u, device=wp_b.device, dtype=torch.int16)
        table = torch.tensor([[0, 2 * h // 16, h]], dtype=torch.int64, device=wp_b.device)
        call("glowtts_wino_weights", ptr(wp_b), wp_b.numel(), ptr(table), 1, ptr(self.u), n_u)

    def bind(self):
        self.M.hip.conv_bind_planes(self.wp_b, self.planes)
        self.M.hip.conv_bind_wino(self.wp_b, self.u)


def _bwd_data(M, d_xin, wp_b, mask, addend, h=H, bias=None, mask_add=False):
    b, _, t = d_xin.shape
    y = torch.full((b, h, t), float("nan"), device=d_xin.device)
    M.hip.call("glowtts_conv_fwd", M.hip.ptr(d_xin), d_xin.stride(0), M.hip.ptr(wp_b), M.hip.ptr(bias), M.hip.ptr(mask),
               M.hip.ptr(addend), 0 if addend is None else addend.stride(0), M.hip.ptr(y), y.stride(0), b, 2 * h, h, t, 5, 1, 2,
               0, int(mask is not None), int(mask_add))
    return y


@pytest.mark.gpu
@pytest.mark.parametrize("b,t,add,masked", [(32, 400, True, True), (48, 600, True, True), (32, 400, False, False),
                                            (3, 36, True, True), (5, 100, False, True), (7, 52, True, False), (2, 8, True, True)])
def test_winograd_bwd_data_against_fp64(M, b, t, add, masked):
    """Against fp64 at the accuracy of the native fp32 kernel (≤ 3x its error), at the benchmark's shape, configs[4]'s and ragged
    shapes (tile counts that are not a multiple of a workgroup's 32; tiles of two utterances in one workgroup); not bitwise equal to
    the direct bf16x6 kernel it replaces (else it did not run), bitwise equal from launch to launch (whichever half came last)."""
    d_xin, v_in, mask, addend = _problem(b, t, b * 131 + t)
    mask = mask if masked else None
    addend = addend if add else None
    _wp_f, wp_b, _ = M.convops.pack_weight(v_in, None)
    ref = F.conv_transpose1d(d_xin.double(), v_in.double(), padding=2)
    if add:
        ref = ref + addend.double()
    if masked:
        ref = ref * mask.double()[:, None]
    bound = _Bound(M, wp_b)
    out, launched = {}, {}
    for name, mode, wino in (("native", "fp32", 0), ("direct", "bf16x6+wrw", 0), ("winograd", "bf16x6+wrw", 1)):
        M.convops.set_conv_math(mode)
        bound.bind()
        M.hip.set_knob("WINO_BWD", wino)
        before = M.hip.wino_bwd_launches()
        out[name] = _bwd_data(M, d_xin, wp_b, mask, addend)
        torch.cuda.synchronize()
        launched[name] = M.hip.wino_bwd_launches() - before
    again = _bwd_data(M, d_xin, wp_b, mask, addend)
    torch.cuda.synchronize()
    assert launched == {"native": 0, "direct": 0, "winograd": 1}, launched
    scale = float(ref.abs().max())
    err = {k: float((v.double() - ref).abs().max()) / scale for k, v in out.items()}
    assert torch.isfinite(out["winograd"]).all()
    assert not torch.equal(out["winograd"], out["direct"]), "the Winograd kernel did not run"
    assert torch.equal(again, out["winograd"]), "not bitwise reproducible"
    assert err["winograd"] <= 3 * err["native"], err
    assert err["winograd"] < 2e-6, err


@pytest.mark.gpu
def test_winograd_bwd_data_switch_and_shapes_outside_it_take_the_direct_kernel(M):
    """GLOWTTS_WINO_BWD=0, T % 4 != 0, a bias, a masked addend, another row count, and unbound planes: the direct kernel."""
    M.convops.set_conv_math("bf16x6+wrw")

    def launches(fn):
        before = M.hip.wino_bwd_launches()
        y = fn()
        torch.cuda.synchronize()
        assert torch.isfinite(y).all()
        return M.hip.wino_bwd_launches() - before

    d_xin, v_in, mask, addend = _problem(4, 64, 11)
    _wp_f, wp_b, _ = M.convops.pack_weight(v_in, None)
    bound = _Bound(M, wp_b)
    bound.bind()
    assert launches(lambda: _bwd_data(M, d_xin, wp_b, mask, addend)) == 1
    M.hip.set_knob("WINO_BWD", 0)
    assert launches(lambda: _bwd_data(M, d_xin, wp_b, mask, addend)) == 0
    M.hip.set_knob("WINO_BWD", 1)
    bias = torch.zeros(H, device="cuda")
    assert launches(lambda: _bwd_data(M, d_xin, wp_b, mask, addend, bias=bias)) == 0
    assert launches(lambda: _bwd_data(M, d_xin, wp_b, mask, addend, mask_add=True)) == 0
    d2, _, mask2, add2 = _problem(4, 62, 12)
    assert launches(lambda: _bwd_data(M, d2.contiguous(), wp_b, mask2, add2)) == 0
    M.hip.conv_bind_wino(None)
    assert launches(lambda: _bwd_data(M, d_xin, wp_b, mask, addend)) == 0
    h = 128
    d3, v3, mask3, add3 = _problem(2, 64, 13, h=h)
    _f3, wp3, _ = M.convops.pack_weight(v3, None)
    b3 = _Bound(M, wp3, h=h)
    b3.bind()
    assert launches(lambda: _bwd_data(M, d3, wp3, mask3, add3, h=h)) == 0


@pytest.mark.gpu
def test_flow_stack_backward_takes_the_winograd_bwd_data_kernel(M):
    """The flow stack's backward (autograd's thread, the native WN executor) launches the Winograd backward-data kernel once per
    WN layer, and GLOWTTS_WINO_BWD=0 puts the direct kernel back with gradients equal to the rounding of the transforms."""
    from glow_tts_train import models

    torch.manual_seed(5)
    b, t, blocks, layers = 4, 64, 2, 4
    dec = models.FlowSpecDecoder(80, hidden_channels=H, kernel_size=5, dilation_rate=1, n_blocks=blocks, n_layers=layers,
                                 p_dropout=0.0, n_split=4, n_sqz=2).cuda().train()
    y0 = torch.randn(b, 80, t, device="cuda")
    lens = torch.tensor([t, t - 8, t - 20, t // 2], device="cuda")
    mask = (torch.arange(t, device="cuda")[None] < lens[:, None]).float()[:, None]
    with torch.no_grad():
        for f in dec.flows:
            if hasattr(f, "end"):
                f.end.weight.normal_(0, 0.02)
    for p in dec.parameters():
        p.grad = torch.zeros_like(p)
    res = {}
    for wino in (1, 0):
        M.hip.set_knob("WINO_BWD", wino)
        for p in dec.parameters():
            p.grad.zero_()
        y = (y0 * mask).clone().requires_grad_(True)
        z, ld = dec(y, mask)
        before = M.hip.wino_bwd_launches()
        (z.square().sum() + ld.sum()).backward()
        torch.cuda.synchronize()
        res[wino] = (y.grad.clone(), {k: p.grad.clone() for k, p in dec.named_parameters()}, M.hip.wino_bwd_launches() - before)
    assert res[1][2] == blocks * layers, res[1][2]
    assert res[0][2] == 0
    g1, p1, _ = res[1]
    g0, p0, _ = res[0]
    assert not torch.equal(g1, g0)
    assert float((g1 - g0).abs().max()) <= 1e-4 * float(g0.abs().max())
    for k in p0:
        assert float((p1[k] - p0[k]).abs().max()) <= 2e-4 * max(1e-3, float(p0[k].abs().max())), k


@pytest.mark.gpu
def test_benchmark_step_launches_the_winograd_bwd_data_kernel_48_times(M, monkeypatch):
    """One training step of the benchmark's workload (12 flow blocks x 4 WN layers) runs the Winograd backward-data kernel for
    every WN layer's in-conv: 48 launches."""
    import os

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    from glow_tts_train.train import train_batch

    monkeypatch.setattr(sys, "argv", ["bench.py"])
    args = bench.parse()
    model, opt, batch, cfg = bench.build_workload(args, torch.device("cuda:0"), 0)
    train_batch(model, opt, batch, cfg.grad_clip, None)
    torch.cuda.synchronize()
    before = M.hip.wino_bwd_launches()
    train_batch(model, opt, batch, cfg.grad_clip, None)
    torch.cuda.synchronize()
    assert M.hip.wino_bwd_launches() - before == 48


@pytest.mark.gpu
def test_winograd_bwd_data_hand_off_with_fresh_inputs_on_two_streams_under_load(M):
    """Every launch gets inputs the one before it did not have (a combining workgroup that read its partner's partial from an
    EARLIER launch, or a stale line of it, would be caught), on two streams at once (each has its own workspace) while a third
    stream keeps other compute units busy (uneven load); every word of every output is checked against fp64."""
    b, t, k_in, n_launch = 32, 400, 4, 12
    dev = "cuda"
    torch.manual_seed(77)
    v_in = torch.randn(2 * H, H, 5, device=dev) * 0.03
    _wp_f, wp_b, _ = M.convops.pack_weight(v_in, None)
    M.convops.set_conv_math("bf16x6+wrw")
    bound = _Bound(M, wp_b)
    bound.bind()
    M.hip.set_knob("WINO_BWD", 1)
    ins = [_problem(b, t, 1000 + i)[::2] for i in range(k_in)]          # (d_xin, mask) per input set
    _d, _v, _m, addend = _problem(b, t, 999)
    refs = [(F.conv_transpose1d(d.double(), v_in.double(), padding=2) + addend.double()) * m.double()[:, None] for d, m in ins]
    scale = max(float(r.abs().max()) for r in refs)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    load = torch.cuda.Stream()
    a = torch.randn(4096, 4096, device=dev)
    torch.cuda.synchronize()
    before = M.hip.wino_bwd_launches()
    outs = []
    with torch.cuda.stream(load):
        for _ in range(6):
            a = torch.tanh(a @ a * 1e-3)
    for i in range(n_launch):
        for si, s in enumerate(streams):
            j = (i + 2 * si) % k_in                          # the two streams on different inputs, each changing every launch
            with torch.cuda.stream(s):
                outs.append((j, _bwd_data(M, ins[j][0], wp_b, ins[j][1], addend)))
    torch.cuda.synchronize()
    assert M.hip.wino_bwd_launches() - before == 2 * n_launch
    for n, (j, y) in enumerate(outs):
        err = float((y.double() - refs[j]).abs().max()) / scale
        assert err < 2e-6, (n, j, err)


@pytest.mark.gpu
def test_winograd_bwd_planes_follow_the_weights_whatever_the_forward_switch(M):
    """The backward-data kernel's U planes are remade with every packing while GLOWTTS_WINO_BWD is on, also with the forward form
    switched off (GLOWTTS_WINO=0), and are not used when they are older than the weights (both switches off at the packing,
    GLOWTTS_WINO_BWD switched on before the backward): the gradients then match the direct kernel's for the NEW weights."""
    from glow_tts_train import models

    torch.manual_seed(9)
    b, t, blocks, layers = 4, 64, 2, 4
    dec = models.FlowSpecDecoder(80, hidden_channels=H, kernel_size=5, dilation_rate=1, n_blocks=blocks, n_layers=layers,
                                 p_dropout=0.0, n_split=4, n_sqz=2).cuda().train()
    y0 = torch.randn(b, 80, t, device="cuda")
    mask = torch.ones(b, 1, t, device="cuda")
    with torch.no_grad():
        for f in dec.flows:
            if hasattr(f, "end"):
                f.end.weight.normal_(0, 0.02)
    for p in dec.parameters():
        p.grad = torch.zeros_like(p)

    def step(wino_fwd, wino_bwd_at_pack, wino_bwd_at_backward):
        M.hip.set_knob("WINO", wino_fwd)
        M.hip.set_knob("WINO_BWD", wino_bwd_at_pack)
        for p in dec.parameters():
            p.grad.zero_()
        y = y0.clone().requires_grad_(True)
        z, ld = dec(y, mask)
        M.hip.set_knob("WINO_BWD", wino_bwd_at_backward)
        before = M.hip.wino_bwd_launches()
        (z.square().sum() + ld.sum()).backward()
        torch.cuda.synchronize()
        return y.grad.clone(), {k: p.grad.clone() for k, p in dec.named_parameters()}, M.hip.wino_bwd_launches() - before

    def close(r1, r0):
        assert float((r1[0] - r0[0]).abs().max()) <= 1e-4 * float(r0[0].abs().max())
        for k in r0[1]:
            assert float((r1[1][k] - r0[1][k]).abs().max()) <= 2e-4 * max(1e-3, float(r0[1][k].abs().max())), k

    try:
        assert step(1, 1, 1)[2] == blocks * layers                # planes made with both forms on
        with torch.no_grad():                                      # new weights
            for p in dec.parameters():
                p.add_(torch.randn_like(p) * 0.02 * (p.abs().mean() + 1e-3))
        new_bwd = step(0, 1, 1)                                    # forward form off: the backward planes still follow
        assert new_bwd[2] == blocks * layers
        direct = step(0, 0, 0)
        assert direct[2] == 0
        close(new_bwd, direct)
        with torch.no_grad():
            for p in dec.parameters():
                p.add_(torch.randn_like(p) * 0.02 * (p.abs().mean() + 1e-3))
        direct2 = step(0, 0, 0)
        late = step(0, 0, 1)                                       # switched on after the packing: planes are older than the weights
        assert late[2] == 0
        close(late, direct2)
    finally:
        M.hip.set_knob("WINO", 1)
        M.hip.set_knob("WINO_BWD", 1)
