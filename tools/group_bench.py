#!/usr/bin/env python3
"""Cost of parameter groups in the fused update (glowtts_adam_noam_groups) at the benchmark's workload, one GPU, ONE process (boxes
differ by several percent); writes profiles/group_bench.json:
  (a) kernels, over buffers of the optimizer's flat size (numel_padded): glowtts_adam_noam; the grouped entry with ONE default group
      (the price of the look-up: the same seven streams p, g, m, v in, p, m, v out); three live groups (plain / L2 / decoupled decay,
      still seven streams); two groups with the second half frozen (half of the seven streams: a frozen range is not streamed).  HIP
      events, RUNS runs of LAUNCHES launches each, the forms alternating run by run; bytes moved next to each time;
  (b) the whole step: alternating blocks of train_batch with the optimizer's three groups at their defaults (the update is then
      glowtts_adam_noam itself) and with live options (plain / L2 / decoupled), the min-max spread of the blocks of one form next to
      the difference of the means.  The difference is stated only if it exceeds the spread.
Usage: python tools/group_bench.py [runs=5] [launches=50] [steps_per_block=20] [blocks=4]"""
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "glow-tts-train_amd")]
import torch  # noqa: E402

import bench  # noqa: E402
from glow_tts_train import _hip, convops, models  # noqa: E402
from glow_tts_train.train import train_batch  # noqa: E402

runs = int(sys.argv[1]) if len(sys.argv) > 1 else 5
launches = int(sys.argv[2]) if len(sys.argv) > 2 else 50
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
blocks = int(sys.argv[4]) if len(sys.argv) > 4 else 4
sys.argv = [sys.argv[0]]
if not torch.cuda.is_available():
    raise SystemExit("group_bench: needs a GPU (a time taken anywhere else says nothing)")
args = bench.parse()
# the benchmark's model and batch; its optimizer is replaced by one with the same hyper-parameters over three groups of the same
# model (all at their defaults to begin with): the new one takes the parameters, as they stand, into flat buffers of its own
RULES = {"encoder.": {}, "encoder.proj": {}, "decoder.": {}}
model, opt, batch, cfg = bench.build_workload(args, torch.device("cuda:0"), 0)
del opt
_, opt = models.setup_model(cfg, model=model, param_rules=RULES)
convops.weights_changed()
flat = opt._optim
n = flat.numel_padded
assert len(flat.param_groups) == 3 and flat._all_default()

# ---- (a) kernels ---------------------------------------------------------------------------------------------------------------
gen = torch.Generator(device="cuda").manual_seed(0)
p, g, m, v = (torch.randn(n, device="cuda", generator=gen) for _ in range(4))
v.abs_()
state = torch.tensor([1.0, 1.0, 0.0, 0.0], device="cuda")
hyper = (1e-3, 0.9, 0.98, 1e-9, 192.0, 4000.0)
four = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr())
third, half = n // 3 // 64 * 64, n // 2 // 64 * 64
DEFAULT, L2, DECOUPLED, FROZEN = (1.0, 0.0, 0.0, 0.0), (1.0, 1e-2, 0.0, 0.0), (1.0, 1e-2, 1.0, 0.0), (1.0, 0.0, 0.0, 1.0)


def plain():
    _hip.call("glowtts_adam_noam", *four, n, state.data_ptr(), *hyper)


def grouped(ends, options):
    end = (ctypes.c_int64 * len(ends))(*ends)
    opts = (ctypes.c_float * (4 * len(ends)))(*[x for o in options for x in o])

    def launch():
        _hip.call("glowtts_adam_noam_groups", *four, None, n, state.data_ptr(), None, *hyper, 0.0, 0, 0.0, ctypes.addressof(end),
                  ctypes.addressof(opts), len(ends))
    return launch


forms = {"adam": plain, "groups_1_default": grouped((n,), (DEFAULT,)),
         "groups_3_live": grouped((third, 2 * third, n), (DEFAULT, L2, DECOUPLED)),
         "groups_half_frozen": grouped((half, n), (DEFAULT, FROZEN))}
floats = {"adam": 7 * n, "groups_1_default": 7 * n, "groups_3_live": 7 * n, "groups_half_frozen": 7 * half}
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
assert bool(torch.isfinite(p).all())
med = {k: statistics.median(ts) for k, ts in us.items()}
print(f"group_bench kernels: n = {n} floats ({4e-6 * n:.1f} MB per stream), {runs} runs x {launches} launches, us per launch")
for k, ts in us.items():
    print(f"  {k:18s} " + "  ".join(f"{t:8.2f}" for t in ts) + f"   median {med[k]:8.2f}  min {min(ts):8.2f}  max {max(ts):8.2f}"
          f"   {4e-6 * floats[k]:.1f} MB moved, {4e-6 * floats[k] / med[k]:.2f} TB/s")
spread = (max(us["adam"]) - min(us["adam"])) / med["adam"]
print(f"  over glowtts_adam_noam: one default group {med['groups_1_default'] / med['adam']:.3f}, three live groups "
      f"{med['groups_3_live'] / med['adam']:.3f}, second half frozen {med['groups_half_frozen'] / med['adam']:.3f} (from the bytes: "
      f"{half / n:.3f}); the plain kernel's own min-max spread: {100 * spread:.2f} %")

# ---- (b) the whole step, the three groups at defaults / with live options, alternating -----------------------------------------
LIVE = ({}, {"weight_decay": 1e-2}, {"weight_decay": 1e-2, "decoupled_weight_decay": True})
for _ in range(8):
    train_batch(model, opt, batch, cfg.grad_clip, None)
res = {"default": [], "groups": []}
for blk in range(2 * blocks):
    mode = ("default", "groups")[blk % 2]
    for group, live in zip(flat.param_groups, LIVE):
        group["weight_decay"] = live.get("weight_decay", 0.0) if mode == "groups" else 0.0
        group["decoupled_weight_decay"] = live.get("decoupled_weight_decay", False) if mode == "groups" else False
    assert flat._all_default() == (mode == "default")
    for _ in range(3):
        train_batch(model, opt, batch, cfg.grad_clip, None)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        train_batch(model, opt, batch, cfg.grad_clip, None)
    torch.cuda.synchronize()
    res[mode].append(1e3 * (time.perf_counter() - t0) / steps)
assert bool(torch.isfinite(flat.flat_p).all())
mean = {k: sum(ts) / len(ts) for k, ts in res.items()}
step_spread = max(max(ts) - min(ts) for ts in res.values())
diff = mean["groups"] - mean["default"]
print(f"group_bench step: B={batch[0].shape[0]} T_text={batch[0].shape[1]} T_mel={batch[2].shape[2]}, {blocks} blocks x {steps} steps per form, ms per step")
for mode, ts in res.items():
    print(f"  {mode:8s}: " + "  ".join(f"{t:.3f}" for t in ts) + f"   mean {mean[mode]:.3f}  min {min(ts):.3f}  max {max(ts):.3f}")
if abs(diff) > step_spread:
    print(f"  groups - default: {diff:+.3f} ms per step (spread of the blocks of one form: {step_spread:.3f} ms)")
else:
    print(f"  groups - default: within the spread of the blocks of one form ({step_spread:.3f} ms): no difference to state")

out = {
    "numel_padded": n, "mb_per_stream": 4e-6 * n, "runs": runs, "launches": launches,
    "group_ends": [int(e) for e in flat.group_ends],
    "kernel_us": {k: {"runs": ts, "median": med[k], "mb_moved": 4e-6 * floats[k]} for k, ts in us.items()},
    "one_default_group_over_plain": med["groups_1_default"] / med["adam"],
    "three_live_groups_over_plain": med["groups_3_live"] / med["adam"],
    "half_frozen_over_plain": med["groups_half_frozen"] / med["adam"], "half_frozen_expected_from_bytes": half / n,
    "plain_spread": spread,
    "step_ms": {"shape": [int(batch[0].shape[0]), int(batch[0].shape[1]), int(batch[2].shape[2])], "steps_per_block": steps,
                "default": res["default"], "groups": res["groups"], "mean_default": mean["default"], "mean_groups": mean["groups"],
                "spread": step_spread, "groups_minus_default": diff if abs(diff) > step_spread else None},
}
path = os.path.join(ROOT, "profiles", "group_bench.json")
with open(path, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print("wrote", path)
