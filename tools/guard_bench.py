#!/usr/bin/env python3
"""Cost of `skip_nonfinite` (the guarded clip and Adam/Noam kernels) at the benchmark's workload, one GPU, ONE process (boxes differ
by several percent):
  1. kernels: glowtts_clip_grad_value vs _guarded and glowtts_adam_noam vs _guarded over buffers of the optimizer's flat size
     (numel_padded), HIP events, RUNS runs of LAUNCHES launches each, the two forms alternating run by run;
  2. the whole step: alternating blocks of train_batch with the optimizer's guard off / on (tools/ab_flags.py's scheme).
Usage: python tools/guard_bench.py [runs=5] [launches=50] [steps_per_block=20] [blocks=4]"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "glow-tts-train_amd")]
import torch  # noqa: E402

import bench  # noqa: E402
from glow_tts_train import _hip  # noqa: E402
from glow_tts_train.train import train_batch  # noqa: E402

runs = int(sys.argv[1]) if len(sys.argv) > 1 else 5
launches = int(sys.argv[2]) if len(sys.argv) > 2 else 50
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
blocks = int(sys.argv[4]) if len(sys.argv) > 4 else 4
sys.argv = [sys.argv[0]]
args = bench.parse()
model, opt, batch, cfg = bench.build_workload(args, torch.device("cuda:0"), 0)
flat = opt._optim
n = flat.numel_padded
clip = float(cfg.grad_clip)

# ---- 1. kernels ----------------------------------------------------------------------------------------------------------------
gen = torch.Generator(device="cuda").manual_seed(0)
p, g, m, v = (torch.randn(n, device="cuda", generator=gen) for _ in range(4))
g.mul_(2.0 * clip)                                           # values on both sides of the clamp
v.abs_()
state = torch.tensor([1.0, 1.0, 0.0, 0.0], device="cuda")
guard = torch.zeros(4, device="cuda")                        # clean: the guarded kernels do all the work
sumsq = torch.zeros(1, device="cuda")
hyper = (1e-3, 0.9, 0.98, 1e-9, 192.0, 4000.0)
forms = {
    "clip": lambda: _hip.call("glowtts_clip_grad_value", g.data_ptr(), n, clip, sumsq.data_ptr()),
    "clip_guarded": lambda: _hip.call("glowtts_clip_grad_value_guarded", g.data_ptr(), n, 1.0, clip, sumsq.data_ptr(), guard.data_ptr()),
    "adam": lambda: _hip.call("glowtts_adam_noam", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, state.data_ptr(), *hyper),
    "adam_guarded": lambda: _hip.call("glowtts_adam_noam_guarded", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n,
                                      state.data_ptr(), guard.data_ptr(), *hyper),
}
for fn in forms.values():
    for _ in range(5):
        fn()
torch.cuda.synchronize()
us = {k: [] for k in forms}
for _run in range(runs):
    for k, fn in forms.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        b.synchronize()
        us[k].append(1e3 * a.elapsed_time(b) / launches)
assert float(guard[0]) == 0.0 and bool(torch.isfinite(p).all())
print(f"guard_bench kernels: n = {n} floats ({4e-6 * n:.1f} MB per buffer), {runs} runs x {launches} launches, us per launch")
for k, ts in us.items():
    print(f"  {k:13s} " + "  ".join(f"{t:8.2f}" for t in ts) + f"   median {statistics.median(ts):8.2f}  min {min(ts):8.2f}  max {max(ts):8.2f}")
for plain, guarded in (("clip", "clip_guarded"), ("adam", "adam_guarded")):
    a, b = statistics.median(us[plain]), statistics.median(us[guarded])
    spread = (max(us[plain]) - min(us[plain])) / a
    print(f"  {guarded} / {plain}: median {100 * (b / a - 1):+.2f} %   (the unguarded kernel's own min-max spread: {100 * spread:.2f} %; "
          f"accepted: within max(3 %, spread))")

# ---- 2. the whole step, guard off / on alternating -------------------------------------------------------------------------------
own_guard = torch.zeros(4, device="cuda")
for _ in range(8):
    train_batch(model, opt, batch, cfg.grad_clip, None)
res = {"off": [], "on": []}
for blk in range(2 * blocks):
    mode = ("off", "on")[blk % 2]
    flat.guard = own_guard if mode == "on" else None
    for _ in range(3):
        train_batch(model, opt, batch, cfg.grad_clip, None)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        train_batch(model, opt, batch, cfg.grad_clip, None)
    torch.cuda.synchronize()
    res[mode].append(1e3 * (time.perf_counter() - t0) / steps)
flat.guard = None
print(f"guard_bench step: B={batch[0].shape[0]} T_text={batch[0].shape[1]} T_mel={batch[2].shape[2]}, {blocks} blocks x {steps} steps per form, ms per step")
for mode, ts in res.items():
    print(f"  guard {mode:3s}: " + "  ".join(f"{t:.3f}" for t in ts) + f"   mean {sum(ts) / len(ts):.3f}  min {min(ts):.3f}  max {max(ts):.3f}")
print(f"  on - off: {sum(res['on']) / blocks - sum(res['off']) / blocks:+.3f} ms per step; skipped updates: {own_guard.tolist()[1]:.0f}")
