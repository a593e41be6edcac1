#!/usr/bin/env python3
"""The backward-data of the gated 5-tap in-conv (dx = (W_in^T (*) d_xin + dx_next) * mask, M = H = 192, K = 2H = 384) at the
benchmark's shape and configs[4]'s: the direct bf16x6 kernel against its Winograd F(4, 5) form (csrc/convwino.hip,
wino_bwd_kernel), alone on the GPU, back to back, HIP events; then the weight transform of a flow stack's 96 packs.
   python tools/wino_bwd_bench.py [B T' ...]      (default: 32 400 48 600)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "glow-tts-train_amd")]
import torch  # noqa: E402

from glow_tts_train import _hip, convops  # noqa: E402

shapes = [int(a) for a in sys.argv[1:]] or [32, 400, 48, 600]
h = 192
dev = "cuda"
call, ptr = _hip.call, _hip.ptr
convops.set_conv_math("bf16x6+wrw")
torch.manual_seed(0)
NW = 12                                                  # cold weights: a different weight set per launch, as in the step
v_in = [torch.randn(2 * h, h, 5, device=dev) * 0.03 for _ in range(NW)]
packs = [convops.pack_weight(v, None) for v in v_in]
arena = torch.cat([torch.cat([f.reshape(-1), b.reshape(-1)]) for f, b, _ in packs])
n1 = packs[0][0].numel()
planes = torch.empty(3 * arena.numel(), device=dev, dtype=torch.int16)
call("glowtts_conv_split_weights", ptr(arena), arena.numel(), ptr(planes))
_hip.conv_bind_planes(arena, planes)
n_u = _hip.wino_plane_elems(arena.numel())
u = torch.zeros(3 * n_u, device=dev, dtype=torch.int16)
rows = []
for i in range(NW):
    rows += [[2 * i * n1, h // 16, 2 * h], [(2 * i + 1) * n1, 2 * h // 16, h]]
table = torch.tensor(rows, dtype=torch.int64, device=dev)
call("glowtts_wino_weights", ptr(arena), arena.numel(), ptr(table), len(rows), ptr(u), n_u)
_hip.conv_bind_wino(arena, u)
wbs = [arena[(2 * i + 1) * n1:(2 * i + 2) * n1] for i in range(NW)]

for b, t in zip(shapes[0::2], shapes[1::2]):
    xs = [torch.randn(b, 2 * h, t, device=dev) for _ in range(4)]
    adds = [torch.randn(b, h, t, device=dev) for _ in range(4)]
    mask = (torch.rand(b, t, device=dev) > 0.1).float()
    y = torch.empty(b, h, t, device=dev)

    def run(n):
        for i in range(n):
            x, a = xs[i % 4], adds[i % 4]
            call("glowtts_conv_fwd", ptr(x), x.stride(0), ptr(wbs[i % NW]), None, ptr(mask), ptr(a), a.stride(0), ptr(y),
                 y.stride(0), b, 2 * h, h, t, 5, 1, 2, 0, 1, 0)

    for wino in (0, 1, 0, 1):
        _hip.set_knob("WINO_BWD", wino)
        run(10)
        torch.cuda.synchronize()
        before = _hip.wino_bwd_launches()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run(200)
        e1.record()
        torch.cuda.synchronize()
        took = _hip.wino_bwd_launches() - before
        assert took == (200 if wino else 0), took
        name = "Winograd F(4,5), K split in two" if wino else "direct bf16x6                  "
        print(f"{name}: {e0.elapsed_time(e1) * 1e3 / 200:7.2f} us per launch (back to back, B={b}, T'={t}, addend + mask, "
              f"{NW} weight sets)", flush=True)

# the flow stack's weight transform: 48 in-convs, forward and backward packs (96 table rows)
big = torch.cat([arena] * 4)
u_big = torch.zeros(3 * _hip.wino_plane_elems(big.numel()), device=dev, dtype=torch.int16)
t_big = torch.tensor([[r[0] + k * arena.numel(), r[1], r[2]] for k in range(4) for r in rows], dtype=torch.int64, device=dev)
for n_rows, label in ((t_big.shape[0] // 2, "forward packs only (48 rows)"), (t_big.shape[0], "forward + backward packs (96 rows)")):
    tb = t_big[0::2].contiguous() if n_rows < t_big.shape[0] else t_big
    for _ in range(3):
        call("glowtts_wino_weights", ptr(big), big.numel(), ptr(tb), tb.shape[0], ptr(u_big), u_big.numel() // 3)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        call("glowtts_wino_weights", ptr(big), big.numel(), ptr(tb), tb.shape[0], ptr(u_big), u_big.numel() // 3)
    e1.record()
    torch.cuda.synchronize()
    print(f"weight transform, {label}: {e0.elapsed_time(e1) * 1e3 / 20:.2f} us per launch")
_hip.set_knob("WINO_BWD", 1)
