#!/usr/bin/env python3
"""Cost of `ema_decay` (the average of the weights kept by the Adam/Noam kernel) at the benchmark's workload, one GPU, ONE process
(boxes differ by several percent); writes profiles/ema_bench.json:
  (a) kernels, over buffers of the optimizer's flat size (numel_padded): glowtts_adam_noam, glowtts_adam_noam_ema, and what the
      fused form replaces — the plain kernel followed by a separate three-stream pass e += a (p - e) (torch's lerp_, the best a
      host-side EMA over ONE flat buffer could do).  HIP events, RUNS runs of LAUNCHES launches each, the forms alternating run
      by run.  Bytes: the plain kernel moves 7 streams (p, g, m, v in; p, m, v out), the EMA form 9, the separate pass 3;
  (b) the whole step: alternating blocks of train_batch with the optimizer's average off / on (tools/ab_flags.py's scheme), the
      min-max spread of the blocks of one form next to the difference of the means.  The difference is stated only if it exceeds
      the spread.
Usage: python tools/ema_bench.py [runs=5] [launches=50] [steps_per_block=20] [blocks=4]"""
import json
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
if not torch.cuda.is_available():
    raise SystemExit("ema_bench: needs a GPU (a time taken anywhere else says nothing)")
args = bench.parse()
model, opt, batch, cfg = bench.build_workload(args, torch.device("cuda:0"), 0)
flat = opt._optim
n = flat.numel_padded

# ---- (a) kernels ---------------------------------------------------------------------------------------------------------------
gen = torch.Generator(device="cuda").manual_seed(0)
p, g, m, v, e = (torch.randn(n, device="cuda", generator=gen) for _ in range(5))
v.abs_()
state = torch.tensor([1.0, 1.0, 0.0, 0.0], device="cuda")
hyper = (1e-3, 0.9, 0.98, 1e-9, 192.0, 4000.0)
RATE = 1e-3


def plain():
    _hip.call("glowtts_adam_noam", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, state.data_ptr(), *hyper)


def fused():
    _hip.call("glowtts_adam_noam_ema", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), e.data_ptr(), n, state.data_ptr(), None,
              *hyper, RATE, 0, 1.0)


def separate():
    plain()
    e.lerp_(p, RATE)


forms = {"adam": plain, "adam_ema": fused, "adam+lerp": separate}
streams = {"adam": 7, "adam_ema": 9, "adam+lerp": 10}
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
assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(e).all())
med = {k: statistics.median(ts) for k, ts in us.items()}
print(f"ema_bench kernels: n = {n} floats ({4e-6 * n:.1f} MB per stream), {runs} runs x {launches} launches, us per launch")
for k, ts in us.items():
    print(f"  {k:10s} " + "  ".join(f"{t:8.2f}" for t in ts) + f"   median {med[k]:8.2f}  min {min(ts):8.2f}  max {max(ts):8.2f}"
          f"   {streams[k]} streams, {streams[k] * 4e-6 * n / med[k]:.2f} TB/s")
spread = (max(us["adam"]) - min(us["adam"])) / med["adam"]
print(f"  adam_ema / adam: {med['adam_ema'] / med['adam']:.3f} (from the bytes: 9 / 7 = {9 / 7:.3f}); the plain kernel's own min-max "
      f"spread: {100 * spread:.2f} %")
print(f"  adam_ema against adam + a separate three-stream pass: {med['adam_ema']:.2f} vs {med['adam+lerp']:.2f} us"
      + ("" if med["adam_ema"] <= med["adam+lerp"] else "   <-- FINDING: the fused kernel is the slower one"))

# ---- (b) the whole step, average off / on alternating --------------------------------------------------------------------------
for _ in range(8):
    train_batch(model, opt, batch, cfg.grad_clip, None)
opt.enable_ema(0.999)
own_e = flat.flat_e
res = {"off": [], "on": []}
for blk in range(2 * blocks):
    mode = ("off", "on")[blk % 2]
    flat.flat_e = own_e if mode == "on" else None
    for _ in range(3):
        train_batch(model, opt, batch, cfg.grad_clip, None)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        train_batch(model, opt, batch, cfg.grad_clip, None)
    torch.cuda.synchronize()
    res[mode].append(1e3 * (time.perf_counter() - t0) / steps)
flat.flat_e = own_e
assert bool(torch.isfinite(own_e).all()) and not torch.equal(own_e, flat.flat_p)
mean = {k: sum(ts) / len(ts) for k, ts in res.items()}
step_spread = max(max(ts) - min(ts) for ts in res.values())
diff = mean["on"] - mean["off"]
print(f"ema_bench step: B={batch[0].shape[0]} T_text={batch[0].shape[1]} T_mel={batch[2].shape[2]}, {blocks} blocks x {steps} steps per form, ms per step")
for mode, ts in res.items():
    print(f"  average {mode:3s}: " + "  ".join(f"{t:.3f}" for t in ts) + f"   mean {mean[mode]:.3f}  min {min(ts):.3f}  max {max(ts):.3f}")
if abs(diff) > step_spread:
    print(f"  on - off: {diff:+.3f} ms per step (spread of the blocks of one form: {step_spread:.3f} ms)")
else:
    print(f"  on - off: within the spread of the blocks of one form ({step_spread:.3f} ms): no difference to state")

out = {
    "numel_padded": n, "mb_per_stream": 4e-6 * n, "runs": runs, "launches": launches,
    "kernel_us": {k: {"runs": ts, "median": med[k], "streams": streams[k]} for k, ts in us.items()},
    "ema_over_plain": med["adam_ema"] / med["adam"], "expected_from_bytes": 9 / 7,
    "fused_slower_than_separate_pass": bool(med["adam_ema"] > med["adam+lerp"]),
    "step_ms": {"shape": [int(batch[0].shape[0]), int(batch[0].shape[1]), int(batch[2].shape[2])], "steps_per_block": steps,
                "off": res["off"], "on": res["on"], "mean_off": mean["off"], "mean_on": mean["on"], "spread": step_spread,
                "on_minus_off": diff if abs(diff) > step_spread else None},
}
path = os.path.join(ROOT, "profiles", "ema_bench.json")
with open(path, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print("wrote", path)
