#!/usr/bin/env python3
"""Gradient accumulation at the benchmark's workload (config 2 shapes, one GPU), three forms interleaved in ONE process (boxes
differ by several percent), N micro-batches each:
  (a) N plain train_batch steps                      (N updates: the cost per batch without accumulation)
  (b) one train_batches update of N micro-batches    (weights packed once per update: convops.weights_unchanged)
  (c) the same update with reuse_packs=False         (every micro-batch packs for itself)
Prints ms per micro-batch of every timed block, and the launches per update that depend on the weights alone.
Usage: python tools/accum_bench.py [N=8] [blocks=6] [updates_per_block=3]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "glow-tts-train_amd")]
import torch  # noqa: E402

import bench  # noqa: E402
from glow_tts_train import _hip, convops, ops  # noqa: E402
from glow_tts_train.train import train_batch, train_batches  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 8
blocks = int(sys.argv[2]) if len(sys.argv) > 2 else 6
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
sys.argv = [sys.argv[0]]
args = bench.parse()
model, opt, batch, cfg = bench.build_workload(args, torch.device("cuda:0"), 0)
micro = [batch] * N


def form_a():
    for _ in range(N):
        train_batch(model, opt, batch, cfg.grad_clip, None)


def form_b():
    train_batches(model, opt, micro, cfg.grad_clip)


def form_c():
    train_batches(model, opt, micro, cfg.grad_clip, reuse_packs=False)


forms = {"a: N x train_batch": form_a, "b: train_batches, packs reused": form_b, "c: train_batches, reuse off": form_c}

# ---- launches per update that depend on the weights alone (an untimed pass with the modules' `call` wrapped) ------------------
KINDS = {"pack": "glowtts_pack_weight", "wino": "glowtts_wino_weights", "prepare": "glowtts_invconv_prepare"}
counts = dict.fromkeys(KINDS, 0)
real_call = _hip.call


def counting(name, *a, **kw):
    for kind, prefix in KINDS.items():
        if name.startswith(prefix):
            counts[kind] += 1
    return real_call(name, *a, **kw)


for _ in range(4):
    form_a()                                                # warm-up: plans built, allocator settled
form_b()
form_c()
torch.cuda.synchronize()
convops.call = ops.call = counting
census = {}
for label, fn in forms.items():
    for k in counts:
        counts[k] = 0
    fn()
    census[label] = dict(counts)
convops.call = ops.call = real_call
torch.cuda.synchronize()

# ---- timing ------------------------------------------------------------------------------------------------------------------
res = {label: [] for label in forms}
for _blk in range(blocks):
    for label, fn in forms.items():
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        res[label].append(1e3 * (time.perf_counter() - t0) / (reps * N))

print(f"accum_bench: B={batch[0].shape[0]} T_text={batch[0].shape[1]} T_mel={batch[2].shape[2]}, N={N} micro-batches, "
      f"{blocks} blocks x {reps} x N micro-batches per form, conv math {convops.conv_math_name()}")
print("ms per micro-batch, block by block (interleaved a, b, c, a, b, c, ...):")
mean = {}
for label, ts in res.items():
    mean[label] = sum(ts) / len(ts)
    print(f"  ({label:32s}) " + "  ".join(f"{t:.3f}" for t in ts) + f"   mean {mean[label]:.3f}  min {min(ts):.3f}  max {max(ts):.3f}")
a, b, c = (mean[k] for k in forms)
spread_a = max(res["a: N x train_batch"]) - min(res["a: N x train_batch"])
print(f"spread between repeated (a) blocks: {spread_a:.3f} ms")
print(f"(b) - (a): {b - a:+.3f} ms per micro-batch ((b) also runs 1 clip + Adam per N micro-batches where (a) runs N)")
print(f"saving of pack reuse, (c) - (b): {c - b:+.3f} ms per micro-batch = {(c - b) * N:+.3f} ms per update of {N}")
print("launches per update of N micro-batches that depend on the weights alone (Python-side calls; for (a): per N steps):")
for label, cnt in census.items():
    print(f"  ({label:32s}) " + "  ".join(f"{k} {v}" for k, v in cnt.items()))
