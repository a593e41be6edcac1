"""The inner training step (reference: glow_tts_train/train.py:91-162) without its host synchronisations.

The reference pays >= 521 device->host syncs per step (two `loss.item()` plus one `.item()` per parameter tensor in
`clip_grad_value_`); here the loss stays on device, clipping and Adam/Noam are one kernel each over flat buffers,
the alignment search never leaves the GPU, and (with `reducer`) gradient all-reduce overlaps the backward.
`train()` is the reference's epoch loop around it (checkpoint cadence included); batches reach HBM one step ahead
through `dataset.DeviceBatches`.

Gradient accumulation (`train_batches`, `accum_steps=`): one update from N micro-batches, each normalised by its own frames and
tokens, the gradients summed in the flat buffer and averaged inside the clip kernel — what N data-parallel ranks with an AVG
all-reduce compute (DistributedDataParallel, reference __main__.py:268-271) on one GPU; the weights are packed once per update.

Non-finite updates (`skip_nonfinite=`, an optimizer built with `optimize.Adam(..., skip_nonfinite=True)`): the clip pass flags a
gradient that holds a NaN or an Inf and the Adam/Noam kernels skip that update on the device — no host read on the step path;
the epoch's one synchronisation also reads the skip counters (`Adam.sync_from_device`).

Averaged weights (`ema_decay=`, an optimizer built with `optimize.Adam(..., ema_decay=0.999)`): the Adam/Noam kernel also moves an
exponential moving average of the parameters — nothing is added to the step path but one buffer streamed through that kernel;
checkpoints carry the average (`"model_ema"`), `optimizer.swap_ema()` runs the model on it.
"""
from __future__ import annotations

import logging
import time
import typing
from pathlib import Path

import torch

import contextlib

from . import convops
from ._hip import join_side_streams, zero_scope
from .convops import flush_groups
from .utils import clip_grad_value_, duration_loss, mle_loss

_LOGGER = logging.getLogger("glow_tts_train")


def train(train_loader, config, model_dir: Path, model=None, optimizer=None, global_step: int = 1,
          checkpoint_epochs: int = 1, rank: int = 0, reducer=None, accum_steps: int = 1, skip_nonfinite: bool = False,
          ema_decay: typing.Optional[float] = None, ema_warmup: bool = False,
          param_rules: typing.Optional[typing.Mapping[str, dict]] = None):
    """Epoch loop of the reference (train.py:19-88): seed, build or adopt model and optimizer, run `config.epochs`
    passes over `train_loader`, and on rank 0 write `checkpoint_<step>.pth` + `config_<step>.json` into `model_dir`
    every `checkpoint_epochs` epochs.  Returns the final global step.  `accum_steps`: loader batches per update (train_step).
    `skip_nonfinite`: skip updates whose gradient is not finite (train_step); an optimizer built here gets the option switched
    on, one passed in must have been built with it.  `ema_decay` / `ema_warmup`: keep an exponential moving average of the
    weights (optimize.FlatAdam); an optimizer built here gets it switched on, one passed in is taken as it is.  The checkpoints
    of an averaging optimizer carry the average.  `param_rules`: an optimizer built here is built from
    `optimize.named_param_groups(model, param_rules)` (frozen / rate-scaled / decayed parts of the model by name prefix: fine-tuning
    from a base checkpoint); one passed in is taken as it is."""
    from .checkpoint import Checkpoint, save_checkpoint
    from .models import setup_model

    torch.manual_seed(config.seed)
    built_here = optimizer is None
    model, optimizer = setup_model(config, model=model, optimizer=optimizer, param_rules=param_rules)
    assert model is not None and optimizer is not None
    if skip_nonfinite and built_here:
        optimizer._optim.enable_skip_nonfinite()
    if ema_decay is not None and built_here:
        optimizer._optim.enable_ema(ema_decay, ema_warmup)
    model_dir = Path(model_dir)
    for epoch in range(1, config.epochs + 1):
        started = time.perf_counter()
        global_step = train_step(global_step=global_step, epoch=epoch, model=model, optimizer=optimizer, config=config,
                                 train_loader=train_loader, fp16_run=config.fp16_run, reducer=reducer, accum_steps=accum_steps,
                                 skip_nonfinite=skip_nonfinite,
                                 on_loss=lambda e, loss, step: _LOGGER.info(
                                     "Avg. Loss for epoch %s: %s (global step=%s)", e, loss, step))
        if epoch % checkpoint_epochs == 0 and rank == 0:
            path = model_dir / f"checkpoint_{global_step}.pth"
            optimizer.sync_from_device()                    # the saved learning_rate is the device's, skipped updates or not
            save_checkpoint(Checkpoint(model=model, optimizer=optimizer, learning_rate=optimizer.cur_lr,
                                       global_step=global_step, version=config.version), path)
            with open(model_dir / f"config_{global_step}.json", "w") as config_file:
                config.save(config_file)
            _LOGGER.info("Saved checkpoint to %s", path)
        _LOGGER.debug("Epoch %s complete in %s second(s) (global step=%s)", epoch, time.perf_counter() - started,
                      global_step)
    return global_step


def train_batch(model, optimizer, batch, grad_clip: float, reducer=None, scaler=None) -> torch.Tensor:
    """One optimisation step on one already-resident batch; returns the (device) loss tensor, un-synchronised.
    `scaler` (a torch GradScaler, reduced-precision runs only): the reference's sequence train.py:133-141 — scale the loss,
    un-scale the gradients before clipping, let the scaler skip the update on overflow.  An optimizer built with
    `skip_nonfinite` skips a non-finite update on the device instead (no new argument: the step follows the optimizer); the
    two together are refused — two skipping mechanisms would disagree about the step counters."""
    x, x_lengths, y, y_lengths, speaker_ids = batch
    flat = getattr(optimizer, "_optim", optimizer)
    if scaler is not None and getattr(flat, "guard", None) is not None:
        raise ValueError("train_batch: a GradScaler (scaler=...) together with an optimizer built with skip_nonfinite=True: "
                         "the scaler already skips non-finite updates; use one of the two")
    optimizer.zero_grad()
    with zero_scope(y.device):          # the step's atomically-accumulated temporaries share one zero fill
        (z, z_m, z_logs, logdet, z_mask), _, (_attn, logw, logw_) = model(x, x_lengths, y, y_lengths, g=speaker_ids)
        loss = mle_loss(z, z_m, z_logs, logdet, z_mask) + duration_loss(logw, logw_, x_lengths)
        (loss if scaler is None else scaler.scale(loss)).backward()
        join_side_streams()             # the encoder branch ran (forward and backward) on a second stream
        flush_groups()                  # weight gradients still packed in a ConvGroup (none, unless a backward was skipped)
        if reducer is not None:
            reducer.finish()
        loss = loss.detach()
    if scaler is not None:
        scaler.unscale_(flat)
    if not (hasattr(flat, "clip_grad_value_") and flat.clip_grad_value_(grad_clip) is not None):
        clip_grad_value_(model.parameters(), grad_clip)
    if scaler is None:
        optimizer.step()
    else:
        # train.py:140: scaler.step(optimizer._optim).  The reference's wrapper never sees that call, so its Noam counter
        # stands still in fp16 runs; here the schedule lives on the device inside FlatAdam.step and advances
        # with every update that is actually applied — the host mirror follows it: GradScaler.step calls flat.step only
        # when the un-scaled gradients are finite, so the mirror advances exactly when that call happened (a skipped update
        # must not move step_num / cur_lr, which checkpoints save and load_state_dict re-imposes).
        applied = []
        inner_step = flat.step
        flat.step = lambda *a, **k: (applied.append(1), inner_step(*a, **k))[1]
        try:
            scaler.step(flat)
        finally:
            del flat.step                   # drop the instance attribute: the class's method is visible again
        scaler.update()
        if applied and hasattr(optimizer, "_update_learning_rate"):
            optimizer._update_learning_rate()
    return loss


def _accumulate(model, optimizer, batches, reducer=None, reuse_packs: bool = True):
    """The accumulating part of `train_batches`: zero the gradients once, then forward + loss + backward of every micro-batch,
    each adding into the flat gradient buffer (every operator accumulates into `.grad`: include/glowtts_hip.h, conventions).
    Returns the micro-batches' (device) losses.  No clipping, no update."""
    batches = list(batches)
    if not batches:
        raise ValueError("train_batches: no micro-batch given")
    m = len(batches)
    optimizer.zero_grad()
    if m > 1:
        convops.weights_changed(record=reuse_packs)      # micro-batch 0 packs as every step does; the rest of the update reuses it
    losses = []
    with contextlib.ExitStack() as scope:
        for k, (x, x_lengths, y, y_lengths, speaker_ids) in enumerate(batches):
            last = k == m - 1
            if k == 1 and reuse_packs:
                scope.enter_context(convops.weights_unchanged())
            # all but the last backward only accumulate; the last one announces the gradients as a plain step does, so the
            # overlapped all-reduce runs once, on the sum
            defer = reducer.no_sync() if (reducer is not None and not last) else contextlib.nullcontext()
            with defer, zero_scope(y.device):
                (z, z_m, z_logs, logdet, z_mask), _, (_attn, logw, logw_) = model(x, x_lengths, y, y_lengths, g=speaker_ids)
                loss = mle_loss(z, z_m, z_logs, logdet, z_mask) + duration_loss(logw, logw_, x_lengths)
                loss.backward()
                join_side_streams()
                flush_groups()
                if reducer is not None and last:
                    reducer.finish()
                losses.append(loss.detach())
    return losses


def train_batches(model, optimizer, batches, grad_clip: float, reducer=None, *, reuse_packs: bool = True) -> torch.Tensor:
    """ONE optimisation step from a non-empty sequence of already-resident micro-batches (they may differ in B, T_text and
    T_mel); returns the mean of their losses as a device tensor, un-synchronised.

    Every micro-batch's loss is normalised by its own frames and tokens exactly as `train_batch` does and is NOT scaled; the
    gradients add up in the flat buffer and are multiplied by 1 / m inside the clip kernel (glowtts_clip_grad_value_scaled), then
    clamped, then one Adam/Noam update: the arithmetic of m data-parallel ranks whose gradients an AVG all-reduce has averaged.
    The step counters advance once.  One micro-batch issues the launches of `train_batch`.

    What depends on the weights alone (weight norm + packing, bf16 and Winograd planes, W^-1 / log det W) is made by the first
    micro-batch and reused by the others (`convops.weights_unchanged`; `reuse_packs=False` makes every micro-batch redo it).
    With `reducer`, all micro-batches but the last run under `reducer.no_sync()`."""
    losses = _accumulate(model, optimizer, batches, reducer, reuse_packs)
    m = len(losses)
    flat = getattr(optimizer, "_optim", optimizer)
    scale = 1.0 / m
    if not (hasattr(flat, "clip_grad_value_") and flat.clip_grad_value_(grad_clip, scale=scale) is not None):
        clip_grad_value_(model.parameters(), grad_clip, scale=scale)
    optimizer.step()
    return losses[0] if m == 1 else torch.stack(losses).mean()


class GraphedTrainStep:
    """The whole training step (zero_grad .. Adam/Noam) captured once into a hipGraph and replayed per batch.

    Every kernel on the path is asynchronous, allocation-free and reads its step-dependent scalars (Adam step, Noam
    learning rate) from device memory, so one captured graph is valid for every later step; replay removes the host
    launch cost of the ~1 400 kernels of a step.  Batches must keep the shapes of `example_batch` (the reference's
    collate pads to the longest utterance of each batch, so a production loop keeps one graph per padded shape).

    With an optimizer built with `skip_nonfinite` the guarded clip and Adam/Noam kernels are what `train_batch` launches, so
    they are what is captured; `__call__` still advances the host mirror with every replay, whether the device applied the
    update or skipped it, and `optimizer.sync_from_device()` is the reconciliation (call it wherever the host reads the loss).
    """

    def __init__(self, model, optimizer, grad_clip: float, example_batch, warmup: int = 2):
        self.model, self.optimizer, self.grad_clip = model, optimizer, grad_clip
        self.static = tuple(None if t is None else t.clone() for t in example_batch)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                       # warm-up on a side stream, as graph capture requires
            for _ in range(warmup):
                train_batch(model, optimizer, self.static, grad_clip)
        torch.cuda.current_stream().wait_stream(side)
        host_state = (optimizer.step_num, optimizer.cur_lr)   # capture runs the Python of a step but no kernel
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.loss = train_batch(model, optimizer, self.static, grad_clip)
        optimizer.step_num, optimizer.cur_lr = host_state

    def __call__(self, batch=None) -> torch.Tensor:
        if batch is not None:
            for dst, src in zip(self.static, batch):
                if dst is not None and src is not dst:
                    dst.copy_(src, non_blocking=True)
        self.graph.replay()
        self.optimizer._update_learning_rate()               # host mirror of the on-device schedule
        return self.loss


def train_step(global_step: int, epoch: int, model, optimizer, config, train_loader, fp16_run: bool = False,
               scaler=None, reducer=None, on_loss: typing.Optional[typing.Callable] = None, accum_steps: int = 1,
               skip_nonfinite: bool = False) -> int:
    """Same signature and return value as the reference's `train_step` (train.py:91-100).

    `fp16_run` (reference train.py:116-121, 133-141: `autocast()` + GradScaler) selects the reduced-precision form of THIS
    build: the flow decoder keeps its activation tensors in HBM as bf16 (`decoder.io_bf16 = "all"`, models.FlowSpecDecoder)
    with fp32 parameters, log-determinants and accumulation, and the text encoder's attention contractions run on the bf16
    matrix pipe (`MultiHeadAttention.bf16_mma`).  bf16 has fp32's exponent range, so no loss scaling is needed:
    `scaler` may be None; a GradScaler that is passed in is driven exactly as the reference drives it.

    `accum_steps` (not part of the reference signature): loader batches per update.  N > 1 groups the batches N at a time into one
    `train_batches` update (a tail of m < N batches at the end of the epoch makes one update averaged over m); `global_step`
    counts updates, `on_loss` receives the mean over updates.  Not combined with a GradScaler.

    `skip_nonfinite` (not part of the reference signature): the optimizer must have been built with
    `optimize.Adam(..., skip_nonfinite=True)`; an update whose gradient holds a NaN or an Inf is then skipped on the device
    (parameters, moments, Adam step, Noam step and rate stand still) and the epoch goes on.  At the epoch's one sync point
    `optimizer.sync_from_device()` reconciles the host's step mirror, `on_loss` receives the mean over the FINITE losses, a
    warning tells how many updates were skipped, and an epoch in which every update was skipped raises RuntimeError.
    `global_step` counts update attempts as before.  Not combined with a GradScaler."""
    from .dataset import DeviceBatches

    accum_steps = int(accum_steps)
    if accum_steps < 1:
        raise ValueError(f"train_step: accum_steps must be >= 1, got {accum_steps}")
    if accum_steps > 1 and scaler is not None:
        raise ValueError("train_step: accum_steps > 1 together with a GradScaler (scaler=...) is not supported; "
                         "fp16_run without a scaler (bf16 tensors need no loss scaling) is")
    guarded = getattr(getattr(optimizer, "_optim", optimizer), "guard", None) is not None
    if skip_nonfinite and not guarded:
        raise ValueError("train_step: skip_nonfinite=True needs an optimizer built with the option: "
                         "optimize.Adam(params, scheduler, dim_model, ..., skip_nonfinite=True)")
    if guarded and scaler is not None:
        raise ValueError("train_step: a GradScaler (scaler=...) together with an optimizer built with skip_nonfinite=True: "
                         "the scaler already skips non-finite updates; use one of the two")
    skipped_before = optimizer.sync_from_device()["skipped"] if guarded and hasattr(optimizer, "sync_from_device") else 0

    model.train()
    bare = model.module if hasattr(model, "module") else model
    decoder = getattr(bare, "decoder", None)
    before = getattr(decoder, "io_bf16", False)
    if fp16_run and decoder is not None and not before:
        decoder.io_bf16 = "all"
    from .attentions import MultiHeadAttention
    mha = [m for m in bare.modules() if isinstance(m, MultiHeadAttention)] if fp16_run else []
    mha_before = [m.bf16_mma for m in mha]
    for m in mha:
        m.bf16_mma = True
    losses = []
    device = next(model.parameters()).device
    try:
        group = []
        for batch in DeviceBatches(train_loader, device):      # batch k+1 is copied to HBM while step k runs
            if accum_steps == 1:
                losses.append(train_batch(model, optimizer, batch, config.grad_clip, reducer, scaler if fp16_run else None))
                global_step += 1
                continue
            group.append(batch)
            if len(group) == accum_steps:
                losses.append(train_batches(model, optimizer, group, config.grad_clip, reducer))
                global_step += 1
                group = []
        if group:                                               # the epoch's tail: one update averaged over what is left
            losses.append(train_batches(model, optimizer, group, config.grad_clip, reducer))
            global_step += 1
    finally:
        if decoder is not None:
            decoder.io_bf16 = before
        for m, b in zip(mha, mha_before):
            m.bf16_mma = b
    if losses and guarded and hasattr(optimizer, "sync_from_device"):
        stacked = torch.stack(losses)
        finite = torch.isfinite(stacked)
        mean = torch.where(finite, stacked, torch.zeros_like(stacked)).sum() / finite.sum().clamp(min=1)
        skipped = optimizer.sync_from_device()["skipped"] - skipped_before       # the epoch's sync point: counters, then the loss
        if skipped:
            _LOGGER.warning("Epoch %s: %s of %s update(s) skipped (non-finite gradient)", epoch, skipped, len(losses))
        if skipped >= len(losses):
            raise RuntimeError(f"train_step: every update of epoch {epoch} ({len(losses)}) had a non-finite gradient and was "
                               "skipped; the model is not training")
        if on_loss is not None:
            on_loss(epoch, float(mean), global_step)
    elif losses and on_loss is not None:
        on_loss(epoch, float(torch.stack(losses).mean()), global_step)   # ONE sync per epoch
    return global_step
