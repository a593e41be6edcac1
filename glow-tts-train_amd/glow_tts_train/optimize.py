"""Adam with the Noam schedule behind the reference's `optimize.Adam` surface (reference: glow_tts_train/optimize.py),
restructured for MI355X: every parameter, gradient and moment lives in ONE flat fp32 buffer each, so

  * `clip_grad_value_` is one streaming kernel instead of 519 `.item()` host syncs (reference utils.py:126-128),
  * the update is one streaming kernel over 4 x 114.5 MB (12 blocks) instead of ~519 x 4 small launches,
  * gradient buckets for data-parallel all-reduce are plain slices of the flat gradient buffer (parallel.py),
  * the learning rate is derived on device from a step counter, so a captured hipGraph replays correctly,
  * an exponential moving average of the parameters (`ema_decay=`) is one more flat buffer streamed through the same update
    kernel: no second pass over the parameters, no extra launch, no host work on the step path,
  * parameter groups (a rate scale, L2 or decoupled weight decay, "frozen") are contiguous ranges of the flat buffers, all updated
    by that one launch; a frozen range is simply not streamed, and its parameters keep their gradient buffers.
"""
from __future__ import annotations

import contextlib
import ctypes
import math
import typing
import weakref
from operator import is_ as _is

import numpy as np
import torch

from ._hip import CONSTANTS, call, ptr, weights_state

_ALIGN = 64  # elements: every parameter starts on a 256-byte boundary of the flat buffers
MAX_PARAM_GROUPS = CONSTANTS["GLOWTTS_MAX_PARAM_GROUPS"]


def clip_launch(g: torch.Tensor, scale: float, clip_value: float, sumsq: torch.Tensor, guard: typing.Optional[torch.Tensor],
                ptr: typing.Callable) -> tuple:
    """The clip entry point for one gradient buffer and its positional arguments, `call(*clip_launch(...))`: the guarded form when the
    owning optimizer has a `guard` (any scale), else the scaled form when `scale` != 1 (an accumulated gradient), else the plain one.
    Nothing is launched here: FlatAdam.clip_grad_value_ and utils.clip_grad_value_ each issue through their own module's `call`
    and hand in their own module's `ptr` (tests replace the two per module)."""
    if guard is not None:
        return "glowtts_clip_grad_value_guarded", ptr(g), g.numel(), float(scale), float(clip_value), ptr(sumsq), ptr(guard)
    if scale != 1.0:
        return "glowtts_clip_grad_value_scaled", ptr(g), g.numel(), float(scale), float(clip_value), ptr(sumsq)
    return "glowtts_clip_grad_value", ptr(g), g.numel(), float(clip_value), ptr(sumsq)


class FlatAdam(torch.optim.Optimizer):
    """torch.optim.Adam arithmetic (no amsgrad / maximize) over flat buffers, launched through the C ABI.

    `skip_nonfinite` (off by default): an update whose gradient holds a NaN or an Inf is skipped on the device, with no host
    read, so the step stays asynchronous and graph-capturable — the skip GradScaler.step gives the reference's fp16 runs
    (train.py:133-141).  `guard` is then a 4-float device tensor [bad flag of the pending update, updates skipped, skipped
    consecutively, updates applied].  The flag is PRODUCED by the clip pass (`clip_grad_value_` here, `utils.clip_grad_value_`,
    both of `train`'s routes): `step()` skips exactly when a clip since the last step saw a non-finite element, so a caller
    who does not clip gets an unguarded update, as without the option.  The counters are not part of `state_dict()` (the file
    format is the reference's): they restart at zero on resume.

    `ema_decay` (off by default; no reference counterpart): `flat_e`, one more flat buffer, holds an exponential moving average
    of the parameters, e <- e + a (p_new - e), moved by the update kernel itself (glowtts_adam_noam_ema, include/glowtts_hip.h)
    with a = 1 - decay, or with `ema_warmup` a = max(1 - decay, 9 / (10 + k)) for the k-th averaged update.  An update the
    device skips (`skip_nonfinite`) leaves the average and its count alone.  `ema_state_dict` / `swap_ema` hand the averaged
    weights out; `state_dict()` keeps torch's layout (checkpoint.py stores the average under keys of its own).  With the
    option off nothing is allocated and nothing else is launched.

    Parameter groups (`params` a list of torch-style group dicts, at most 8): each group is one contiguous range of the flat
    buffers (the layout is group-major) and may set `weight_decay`, `decoupled_weight_decay` (torch.optim.Adam's own keys: L2
    decay, or AdamW's), `lr_scale` (default 1.0: the group's rate is the shared rate times it, and the group's `lr` is a host
    mirror of that) and `frozen` (default False: the update leaves the range alone and streams nothing of it; the parameters
    keep their gradient buffers, so the native training path and the data-parallel buckets do not notice).  `betas` and `eps` are
    shared.  The options are read at every `step()`, so they may be edited in `param_groups` between updates — but not under a
    captured graph: the table is a by-value argument of the kernel, fixed when the launch is captured, so a replay applies the
    options of the capture and an edit made afterwards is NOT honoured until the step is captured again.  While every
    group is at its defaults, `step()` launches what an optimizer without groups launches; otherwise
    glowtts_adam_noam_groups runs in place of the glowtts_adam_noam* call.  The clip pass does not know groups: the norm and,
    with `skip_nonfinite`, the non-finite test cover the whole gradient buffer, so a NaN in a FROZEN group's gradient still
    skips the update."""

    def __init__(self, params, lr=1.0, betas=(0.9, 0.98), eps=1e-9, dim_model: float = 0.0, warmup_steps: float = 0.0,
                 base_lr: typing.Optional[float] = None, skip_nonfinite: bool = False,
                 ema_decay: typing.Optional[float] = None, ema_warmup: bool = False):
        params = [p for p in params]
        if params and isinstance(params[0], dict):
            if len(params) > MAX_PARAM_GROUPS:
                raise ValueError(f"FlatAdam: {len(params)} parameter groups, the update kernel takes at most {MAX_PARAM_GROUPS}")
            if any("lr" in g for g in params):
                raise ValueError("FlatAdam: a group's rate is the shared rate times its `lr_scale`; `lr` cannot be set per group")
        # the group carries every key torch.optim.Adam's does (amsgrad, weight_decay, foreach, ... at their defaults), so
        # state_dict() has torch's layout for this torch version and the reference loads it unchanged
        template = torch.optim.Adam([torch.zeros(1)], lr=lr, betas=betas, eps=eps).param_groups[0]
        super().__init__(params, {k: v for k, v in template.items() if k != "params"})
        for g in self.param_groups:
            if tuple(g["betas"]) != tuple(self.param_groups[0]["betas"]) or g["eps"] != self.param_groups[0]["eps"]:
                raise ValueError("FlatAdam: betas and eps are shared by all parameter groups")
        for k, (scale, _, _, _) in enumerate(self._group_options()):           # (raises on a negative or non-finite option)
            if scale != 1.0:
                self.param_groups[k]["lr"] = lr * scale                       # host mirror of the group's rate
        self.base_lr = float(lr if base_lr is None else base_lr)
        self.dim_model, self.warmup = float(dim_model), float(warmup_steps)
        self.guard: typing.Optional[torch.Tensor] = None
        self.flat_e: typing.Optional[torch.Tensor] = None
        self.ema_decay: typing.Optional[float] = None
        self.ema_warmup = False
        self._ema_rate, self._ema_t0, self._ema_swapped = 0.0, 0.0, False
        if ema_decay is not None:
            _check_decay(ema_decay)
        self._build_flat()
        if skip_nonfinite:
            self.enable_skip_nonfinite()
        if ema_decay is not None:
            self.enable_ema(ema_decay, ema_warmup)

    # -- layout -------------------------------------------------------------------------------------------------
    def _build_flat(self):
        ps = [p for g in self.param_groups for p in g["params"]]
        if not ps:
            raise ValueError("FlatAdam: no parameters")
        dev, dt = ps[0].device, torch.float32
        offs, total = [], 0
        for p in ps:
            if p.dtype != dt or p.device != dev:
                raise RuntimeError("FlatAdam: all parameters must be fp32 on one device")
            offs.append(total)
            total += (p.numel() + _ALIGN - 1) // _ALIGN * _ALIGN
        self.offsets, self.numel_padded = offs, total
        self.numel = sum(p.numel() for p in ps)
        # the layout is group-major, so every group is ONE range of the flat buffers: group k ends where its last parameter's
        # padding does (multiples of _ALIGN: the update kernel keeps its 16-byte form)
        counts = np.cumsum([len(g["params"]) for g in self.param_groups])
        self.group_ends = [total if c == len(ps) else offs[c] for c in counts]
        # host arrays of glowtts_adam_noam_groups, read during the call only
        self._group_end = (ctypes.c_int64 * len(self.group_ends))(*self.group_ends)
        self._group_opts = (ctypes.c_float * (4 * len(self.group_ends)))()
        self.flat_p = torch.zeros(total, device=dev, dtype=dt)
        self.flat_g = torch.zeros(total, device=dev, dtype=dt)
        self.flat_m = torch.zeros(total, device=dev, dtype=dt)
        self.flat_v = torch.zeros(total, device=dev, dtype=dt)
        # device state: [adam step t (1-based for the NEXT update), noam step_num, lr of the next update,
        #                lr imposed on the next update only (0 = follow the schedule)]
        self.dev_state = torch.tensor([1.0, 1.0, 0.0, 0.0], device=dev, dtype=dt)
        with torch.no_grad():
            for p, o in zip(ps, offs):
                n = p.numel()
                self.flat_p[o:o + n].copy_(p.detach().reshape(-1))
                p.data = self.flat_p[o:o + n].view(p.shape)
                if p.grad is not None:
                    self.flat_g[o:o + n].copy_(p.grad.reshape(-1))
                p.grad = self.flat_g[o:o + n].view(p.shape)
                p._glowtts_flat_grad = self.flat_g
                p._glowtts_flat_numel = self.numel
                p._glowtts_flat_owner = weakref.ref(self)
        self._params = ps
        # zero_grad() has not run yet: the views just installed are the ones grads_in_place() compares against
        self._views = [p.grad for p in ps]

    def enable_skip_nonfinite(self) -> None:
        """Switch `skip_nonfinite` on for an optimizer built without it (train.train does, for the optimizer it built itself):
        allocates `guard`; from the next clip pass on, the guarded kernels run."""
        if self.guard is None:
            self.guard = torch.zeros(4, device=self.flat_p.device, dtype=torch.float32)

    def slices(self):
        """(offset, numel) of every parameter inside the flat buffers, in construction order."""
        return [(o, p.numel()) for p, o in zip(self._params, self.offsets)]

    # -- parameter groups ---------------------------------------------------------------------------------------
    def _group_options(self) -> typing.List[typing.Tuple[float, float, bool, bool]]:
        """(lr_scale, weight_decay, decoupled, frozen) of every group, as the groups say NOW (they may be edited between updates);
        a negative or non-finite lr_scale / weight_decay raises ValueError."""
        out = []
        for k, g in enumerate(self.param_groups):
            scale, decay = float(g.get("lr_scale", 1.0)), float(g["weight_decay"])
            if not (math.isfinite(scale) and math.isfinite(decay) and scale >= 0.0 and decay >= 0.0):
                raise ValueError(f"FlatAdam: group {k}: lr_scale = {scale} and weight_decay = {decay} must be finite and >= 0")
            out.append((scale, decay, bool(g.get("decoupled_weight_decay", False)), bool(g.get("frozen", False))))
        return out

    def _all_default(self) -> bool:
        """Every group at lr_scale 1, no decay, not frozen: the update is the one an optimizer without groups launches."""
        for g in self.param_groups:
            if g["weight_decay"] != 0 or g.get("lr_scale", 1.0) != 1.0 or g.get("frozen", False):
                return False
        return True

    # -- exponential moving average of the parameters -----------------------------------------------------------
    def enable_ema(self, decay: float, warmup: bool = False, num_updates: int = 0) -> None:
        """Switch the average on (once: a second call raises): `flat_e` starts as a copy of `flat_p`, padding included, and the
        updates from now on move it.  `num_updates`: averaged updates already behind this average (a resumed run) — the warm-up
        continues from there.  Reads the device's Adam step once; the count is kept as the step the average started at, so no
        state of its own lives on the device.

        Call it AFTER a data-parallel broadcast of the parameters (parallel.FlowBlockReducer.broadcast_parameters): the ranks'
        averages start from the copy made here and then see the same updates, so they stay bit-equal only if the parameters
        were already the same when it was made."""
        if self.flat_e is not None:
            raise RuntimeError("FlatAdam.enable_ema: the average is already on")
        decay = _check_decay(decay)
        num_updates = int(num_updates)
        if num_updates < 0:
            raise ValueError(f"FlatAdam.enable_ema: num_updates must be >= 0, got {num_updates}")
        self.ema_decay, self.ema_warmup = decay, bool(warmup)
        self._ema_rate = 1.0 - decay                        # fp64 here, rounded to fp32 once at the call (1 - fl32(decay) is not this)
        self._ema_t0 = float(self.dev_state[0]) - num_updates
        self.flat_e = self.flat_p.clone()

    def _need_ema(self, who: str) -> None:
        if self.flat_e is None:
            raise RuntimeError(f"FlatAdam.{who}: the optimizer was built without ema_decay (enable_ema switches it on)")

    def ema_num_updates(self) -> int:
        """Updates the average has seen (ONE device read); an update the device skipped is not among them."""
        self._need_ema("ema_num_updates")
        return int(round(float(self.dev_state[0]) - self._ema_t0))

    def _owned(self, tensor: torch.Tensor) -> typing.Optional[int]:
        """Offset in the flat buffers of the parameter `tensor` is a view of (a state_dict entry shares its parameter's storage),
        None for anything else."""
        by_offset = getattr(self, "_numel_at", None)
        if by_offset is None:
            by_offset = self._numel_at = {o: p.numel() for p, o in zip(self._params, self.offsets)}
        if tensor.device != self.flat_p.device or tensor.dtype != torch.float32 or tensor.numel() == 0:
            return None
        delta = tensor.data_ptr() - self.flat_p.data_ptr()
        if delta < 0 or delta % 4 or by_offset.get(delta // 4) != tensor.numel():
            return None
        return delta // 4

    def ema_state_dict(self, model) -> dict:
        """`model.state_dict()` with every parameter this optimizer owns replaced by its averaged value (a clone); every other
        entry (buffers, parameters of another optimizer) is copied.  Keys, their order and the shapes are the model's."""
        self._need_ema("ema_state_dict")
        averaged = self.flat_p if self._ema_swapped else self.flat_e          # inside swap_ema() the two have changed places
        out = {}
        for key, value in model.state_dict().items():
            o = self._owned(value)
            out[key] = (value if o is None else averaged[o:o + value.numel()].view(value.shape)).detach().clone()
        return out

    def load_ema_state_dict(self, model, averaged: dict, num_updates: typing.Optional[int] = None) -> None:
        """The inverse of `ema_state_dict`: fill `flat_e` from `averaged` (entries of parameters this optimizer does not own are
        ignored, a missing or mis-shaped one raises) and, if given, continue the count at `num_updates`."""
        self._need_ema("load_ema_state_dict")
        if self._ema_swapped:
            raise RuntimeError("FlatAdam.load_ema_state_dict inside swap_ema()")
        with torch.no_grad():
            for key, value in model.state_dict().items():
                o = self._owned(value)
                if o is None:
                    continue
                if key not in averaged or tuple(averaged[key].shape) != tuple(value.shape):
                    raise ValueError(f"averaged weights: no entry of shape {tuple(value.shape)} for {key}")
                self.flat_e[o:o + value.numel()].copy_(averaged[key].reshape(-1))
        if num_updates is not None:
            self._ema_t0 = float(self.dev_state[0]) - int(num_updates)

    @contextlib.contextmanager
    def swap_ema(self):
        """`with opt.swap_ema():` — the model runs on the averaged weights (validation, synthesis): `flat_p` and `flat_e` are
        exchanged by one kernel on entry and again on exit; the parameters stay views of `flat_p`, so no pointer moves and no
        module is touched.  Both exchanges call `convops.weights_changed()`: nothing packed from the other weights is reused.
        Inside the scope `step()`, `enable_ema`, a nested `swap_ema()` and `checkpoint.save_checkpoint` raise; entering it inside
        `convops.weights_unchanged()` raises."""
        self._need_ema("swap_ema")
        if self._ema_swapped:
            raise RuntimeError("FlatAdam.swap_ema: already inside swap_ema()")
        if weights_state.active:
            raise RuntimeError("FlatAdam.swap_ema inside convops.weights_unchanged(): the scope must end before the weights change")
        self._exchange()
        self._ema_swapped = True
        try:
            yield self
        finally:
            self._exchange()
            self._ema_swapped = False

    def _exchange(self) -> None:
        from .convops import weights_changed

        call("glowtts_swap_f32", ptr(self.flat_p), ptr(self.flat_e), self.numel_padded)
        weights_changed()

    # -- torch.optim surface ------------------------------------------------------------------------------------
    def _grad_views(self):
        """The gradient views handed out by zero_grad, kept so that "is .grad still ours?" is an identity test per
        parameter (this runs three times per step over ~500 parameters: pointer arithmetic there cost milliseconds)."""
        views = getattr(self, "_views", None)
        if views is None:
            views = self._views = [None] * len(self._params)
        return views

    def zero_grad(self, set_to_none: bool = False):
        # the gradients must stay views of the flat buffer: one memset, never `grad = None`
        self.flat_g.zero_()
        views = self._grad_views()
        for i, p in enumerate(self._params):
            if p.grad is not views[i] or views[i] is None:
                o = self.offsets[i]
                views[i] = self.flat_g[o:o + p.numel()].view(p.shape)
                p.grad = views[i]

    def grads_in_place(self) -> bool:
        views = self._grad_views()
        return all(map(_is, [p.grad for p in self._params], views))        # (C-level loops: called twice per step)

    def clip_grad_value_(self, clip_value: float, scale: float = 1.0):
        """utils.clip_grad_value_ over the whole flat gradient buffer in one launch; None if a gradient has been replaced by
        a foreign tensor (the caller then takes the general path).  `scale` != 1: the buffer holds a SUM of micro-batch
        gradients (train.train_batches) and is multiplied by `scale` in the same pass, before the norm and the clamp.
        With `skip_nonfinite` the pass also sets guard[0] when an element of the scaled gradient is not finite."""
        if not self.grads_in_place():
            return None
        from .utils import _FlatGradView
        sumsq = torch.zeros(1, device=self.flat_g.device, dtype=torch.float32)
        call(*clip_launch(self.flat_g, scale, clip_value, sumsq, self.guard, ptr))
        return _FlatGradView(sumsq, 2.0)

    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            raise NotImplementedError("FlatAdam.step: closures are not supported")
        if weights_state.active:                      # (convops.weights_unchanged: packed weights are being reused as they are)
            raise RuntimeError("FlatAdam.step inside convops.weights_unchanged(): the scope must end before the weights change")
        if self._ema_swapped:
            raise RuntimeError("FlatAdam.step inside swap_ema(): the parameters hold the averaged weights")
        if not self.grads_in_place():                 # a foreign hook may have replaced .grad: fold it back in
            views = self._grad_views()
            for i, (p, o) in enumerate(zip(self._params, self.offsets)):
                if p.grad is not None and p.grad is not views[i] and p.grad.data_ptr() != self.flat_g.data_ptr() + 4 * o:
                    self.flat_g[o:o + p.numel()].copy_(p.grad.reshape(-1))
                if p.grad is not views[i]:
                    views[i] = self.flat_g[o:o + p.numel()].view(p.shape)
                    p.grad = views[i]
        g = self.param_groups[0]
        b1, b2 = g["betas"]
        buffers = (ptr(self.flat_p), ptr(self.flat_g), ptr(self.flat_m), ptr(self.flat_v))
        rates = (self.base_lr, float(b1), float(b2), float(g["eps"]), self.dim_model, self.warmup)
        guarded = "_guarded" if self.guard is not None else ""
        guard = (ptr(self.guard),) if guarded else ()
        if not self._all_default():                   # some group has options of its own: the grouped form of the same update
            for k, (scale, decay, decoupled, frozen) in enumerate(self._group_options()):
                self._group_opts[4 * k: 4 * k + 4] = (scale, decay, float(decoupled), float(frozen))
            call("glowtts_adam_noam_groups", *buffers, ptr(self.flat_e), self.numel_padded, ptr(self.dev_state), ptr(self.guard),
                 *rates, self._ema_rate, int(self.ema_warmup), self._ema_t0, ctypes.addressof(self._group_end),
                 ctypes.addressof(self._group_opts), len(self.group_ends))
        elif self.flat_e is not None:                 # the same update with the average carried along; its guard may be NULL
            call("glowtts_adam_noam_ema", *buffers, ptr(self.flat_e), self.numel_padded, ptr(self.dev_state), ptr(self.guard), *rates,
                 self._ema_rate, int(self.ema_warmup), self._ema_t0)
        else:
            call("glowtts_adam_noam" + guarded, *buffers, self.numel_padded, ptr(self.dev_state), *guard, *rates)
        call("glowtts_adam_advance" + guarded, ptr(self.dev_state), *guard, self.base_lr, self.dim_model, self.warmup)

    def state_dict(self):
        """torch.optim.Adam-compatible layout: state[i] = {step, exp_avg, exp_avg_sq} (what checkpoint.py:44 saves).  The
        `skip_nonfinite` counters (`guard`) are not saved, and neither is the averaged copy of the weights (`ema_state_dict`;
        checkpoint.py writes it under keys of its own): the layout is torch's with the option on or off."""
        t = (self.dev_state[0] - 1.0).detach().cpu()        # ONE device read for the step every entry shares
        state = {}
        for i, (p, o) in enumerate(zip(self._params, self.offsets)):
            n = p.numel()
            state[i] = {
                "step": t.clone(),
                "exp_avg": self.flat_m[o:o + n].view(p.shape).clone(),
                "exp_avg_sq": self.flat_v[o:o + n].view(p.shape).clone(),
            }
        groups = [{k: v for k, v in g.items() if k != "params"} for g in self.param_groups]
        # `lr_scale` / `frozen` are this package's keys: a file carries them only when some group uses one (then every group
        # does), so an optimizer without them writes exactly torch.optim.Adam's keys
        special = any(g.get("lr_scale", 1.0) != 1.0 or g.get("frozen", False) for g in groups)
        first = 0
        for g, own in zip(groups, self.param_groups):
            scale, frozen = g.pop("lr_scale", 1.0), g.pop("frozen", False)
            if special:
                g["lr_scale"], g["frozen"] = float(scale), bool(frozen)
            g["params"] = list(range(first, first + len(own["params"])))       # group-major, as torch numbers them
            first += len(own["params"])
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, d):
        """Like torch.optim.Optimizer.load_state_dict: a state whose parameter count or moment shapes differ from this
        optimizer's raises ValueError; an EMPTY state (a file saved before the first update) is accepted, and so is a
        state without an entry for some parameter — torch.optim.Adam only creates a parameter's state at its first
        gradient, so a reference checkpoint of a model with a frozen / never-used parameter has none: zero moments here,
        with a warning.  A state of ONE group loads into an optimizer of several (its moments by parameter index; this
        optimizer's group options stay); several groups in the file must be as many as here and hold as many parameters
        each, else ValueError.  With as many groups as here the FILE's options win, a missing `lr_scale` / `frozen` included:
        state_dict() writes the two only when some group uses one, so their absence says 1.0 / False."""
        st = d.get("state", {})
        saved_groups = d.get("param_groups", [])
        # the average counts its updates from the device's Adam step, which this call may move: the count itself stays
        ema_seen = self.ema_num_updates() if self.flat_e is not None else None
        if len(saved_groups) > 1 and len(saved_groups) != len(self.param_groups):
            raise ValueError(f"loaded state dict has {len(saved_groups)} parameter groups, the optimizer has {len(self.param_groups)}: "
                             "only a single-group state can be spread over other groups")
        if saved_groups and "params" in saved_groups[0]:
            n_saved = sum(len(g["params"]) for g in saved_groups)
            if n_saved != len(self._params):
                raise ValueError(f"loaded state dict has {n_saved} parameters, the optimizer has {len(self._params)}")
            # several groups: the file's options belong to the parameters they were saved for (torch.optim raises here too)
            sizes, own_sizes = [len(g["params"]) for g in saved_groups], [len(g["params"]) for g in self.param_groups]
            if len(saved_groups) > 1 and sizes != own_sizes:
                raise ValueError(f"loaded state dict has parameter groups of {sizes} parameters, the optimizer's have {own_sizes}")
        same_groups = len(saved_groups) == len(self.param_groups)
        missing = [i for i in range(len(self._params)) if st and i not in st and str(i) not in st]
        if missing:
            import warnings
            warnings.warn(f"FlatAdam.load_state_dict: no state for parameters {missing[:8]}{'...' if len(missing) > 8 else ''} "
                          "(never updated when the file was written): their moments start at zero.  All parameters share ONE "
                          "device step counter here, so these parameters' bias correction continues at the file's step N — "
                          "torch.optim.Adam would restart theirs at step 1 (their first updates are ~1 / (1 - beta1^N) times "
                          "smaller than the reference's)")
        steps = []
        with torch.no_grad():
            for i, (p, o) in enumerate(zip(self._params, self.offsets)):
                s = st.get(i, st.get(str(i)))
                n = p.numel()
                if s is None:
                    if st:
                        self.flat_m[o:o + n].zero_()
                        self.flat_v[o:o + n].zero_()
                    continue
                for name in ("exp_avg", "exp_avg_sq"):
                    if tuple(s[name].shape) != tuple(p.shape):
                        raise ValueError(f"optimizer state {name}[{i}] has shape {tuple(s[name].shape)}, "
                                         f"the parameter has {tuple(p.shape)}")
                self.flat_m[o:o + n].copy_(s["exp_avg"].reshape(-1))
                self.flat_v[o:o + n].copy_(s["exp_avg_sq"].reshape(-1))
                steps.append(float(s["step"]))
            if steps:
                if max(steps) != min(steps):
                    import warnings
                    warnings.warn("FlatAdam.load_state_dict: per-parameter steps differ; using the largest")
                self.dev_state[0] = max(steps) + 1.0
                if ema_seen is not None:
                    self._ema_t0 = max(steps) + 1.0 - ema_seen
        # The groups.  As many in the file as here: every group takes its options from the file.  ONE group in the file and several
        # here (fine-tuning from a base checkpoint): the file's moments were matched by index above, its betas / eps are shared, and
        # the options this optimizer was built with stay.
        if same_groups:
            for g_new, g in zip(saved_groups, self.param_groups):
                for k in ("lr", "betas", "eps", "weight_decay", "decoupled_weight_decay"):
                    if k in g_new:
                        g[k] = g_new[k]
                # state_dict() leaves these two out when every group has them at their defaults (and a file of the reference or
                # from before the groups never has them): absent means 1.0 / False, not "keep this optimizer's"
                for k in ("lr_scale", "frozen"):
                    if k in g_new:
                        g[k] = g_new[k]
                    else:
                        g.pop(k, None)
        elif len(saved_groups) == 1:
            for g in self.param_groups:
                for k in ("betas", "eps"):
                    if k in saved_groups[0]:
                        g[k] = saved_groups[0][k]
        options = self._group_options()
        # torch.optim.Adam.load_state_dict leaves the stored group lr in force until the schedule next writes it, i.e.
        # for exactly one update under "noam" (reference optimize.py:43-48, :60-61) and for good otherwise.  What is imposed is
        # a BASE rate (the kernel scales it per group): the stored rate of the first live group with a rate, over the lr_scale
        # it was SAVED at (the file's, which with as many groups as here is now this optimizer's too; 1.0 for a one-group file
        # spread over several).  Every group's `lr` mirror is then that base rate times the group's own scale: what the kernel
        # applies, whatever the file's other `lr` entries say.
        saved_options = options if same_groups else [(1.0, 0.0, False, False)] * len(saved_groups)
        for g_new, (saved_scale, _, _, frozen) in zip(saved_groups, saved_options):
            if "lr" in g_new and saved_scale > 0.0 and not frozen:
                saved_lr = float(g_new["lr"])
                lr = saved_lr / saved_scale
                if self.warmup > 0.0:
                    self.dev_state[3] = lr
                else:
                    self.base_lr = lr
                for g, (scale, _, _, _) in zip(self.param_groups, options):
                    g["lr"] = saved_lr if scale == saved_scale else lr * scale     # (x / s * s need not be x)
                break


def _check_decay(decay) -> float:
    decay = float(decay)
    if not 0.0 < decay < 1.0:
        raise ValueError(f"ema_decay must lie strictly between 0 and 1, got {decay}")
    return decay


class Adam:
    """Reference surface (optimize.py:8-64): `Adam(params, scheduler, dim_model, warmup_steps, lr, betas, eps)` with
    `.step() .zero_grad() .get_lr() .state_dict() .load_state_dict() .cur_lr .step_num ._optim`.  Keyword-only additions:
    `skip_nonfinite`, `ema_decay`, `ema_warmup` (FlatAdam); `enable_ema`, `ema_num_updates`, `ema_state_dict` and `swap_ema`
    are FlatAdam's.  `params` may be a list of parameter-group dicts (FlatAdam; `named_param_groups` builds one from name
    prefixes): every group's `lr` then mirrors `cur_lr` times its `lr_scale`."""

    def __init__(self, params, scheduler, dim_model, warmup_steps: int = 4000, lr: float = 1e0,
                 betas: typing.Tuple[float, float] = (0.9, 0.98), eps: float = 1e-9, *, skip_nonfinite: bool = False,
                 ema_decay: typing.Optional[float] = None, ema_warmup: bool = False):
        self.params = list(params)
        self.scheduler, self.dim_model, self.warmup_steps = scheduler, dim_model, warmup_steps
        self.lr, self.betas, self.eps = lr, betas, eps
        self.step_num = 1
        self.cur_lr = lr * self._get_lr_scale()
        noam = scheduler == "noam"
        self._optim = FlatAdam(self.params, lr=self.cur_lr, betas=betas, eps=eps, base_lr=lr,
                               dim_model=dim_model if noam else 0.0, warmup_steps=warmup_steps if noam else 0.0,
                               skip_nonfinite=skip_nonfinite, ema_decay=ema_decay, ema_warmup=ema_warmup)

    def _get_lr_scale(self):
        if self.scheduler == "noam":
            return np.power(self.dim_model, -0.5) * np.min(
                [np.power(self.step_num, -0.5), self.step_num * np.power(self.warmup_steps, -1.5)])
        return 1

    def _update_learning_rate(self):
        # host mirror of what glowtts_adam_advance did on device (no synchronisation)
        self.step_num += 1
        if self.scheduler == "noam":
            self.cur_lr = self.lr * self._get_lr_scale()
            for group in self._optim.param_groups:
                group["lr"] = self.cur_lr * group.get("lr_scale", 1.0)

    def get_lr(self):
        return self.cur_lr

    def step(self):
        self._optim.step()
        self._update_learning_rate()

    def zero_grad(self):
        self._optim.zero_grad()

    def enable_ema(self, decay: float, warmup: bool = False, num_updates: int = 0) -> None:
        self._optim.enable_ema(decay, warmup, num_updates)

    def ema_num_updates(self) -> int:
        return self._optim.ema_num_updates()

    def ema_state_dict(self, model) -> dict:
        return self._optim.ema_state_dict(model)

    def swap_ema(self):
        return self._optim.swap_ema()

    def sync_from_device(self) -> typing.Dict[str, int]:
        """ONE device-to-host copy of the device's step state and the `skip_nonfinite` counters; sets `step_num`, `cur_lr` and
        `param_groups[...]["lr"]` to the device's values and returns {"applied", "skipped", "consecutive_skipped"} (updates since
        construction; they are not saved in checkpoints and restart at zero on resume).

        `step()` (and GraphedTrainStep) advance the host mirror with every update ATTEMPT without asking the device; an update
        the device skipped leaves the mirror one step ahead, and this call is the reconciliation.  Without `skip_nonfinite`
        the skip counts are zero and the mirror already agrees: a no-op on a healthy run."""
        flat = self._optim
        if flat.guard is None:
            host = flat.dev_state.detach().cpu().tolist() + [0.0] * 4
        else:
            host = torch.cat([flat.dev_state.detach(), flat.guard.detach()]).cpu().tolist()
        if int(host[1]) != self.step_num:            # the mirror ran ahead: the schedule is re-derived from the device's step
            self.step_num = int(host[1])
            if self.scheduler == "noam":
                self.cur_lr = self.lr * self._get_lr_scale()
                for group in flat.param_groups:
                    # a rate a resumed checkpoint imposed on the next update (dev_state[3]) is still pending after a skip
                    group["lr"] = (host[3] if host[3] > 0.0 else self.cur_lr) * group.get("lr_scale", 1.0)
        return {"applied": int(host[7]), "skipped": int(host[5]), "consecutive_skipped": int(host[6])}

    def load_state_dict(self, d):
        """The `skip_nonfinite` counters are not part of the file: they keep their values (zero after construction)."""
        self._optim.load_state_dict(d)

    def state_dict(self):
        return self._optim.state_dict()


def named_param_groups(model: torch.nn.Module, rules: typing.Optional[typing.Mapping[str, dict]],
                       default: typing.Optional[dict] = None) -> typing.List[dict]:
    """Parameter groups for `Adam` / `FlatAdam` from name prefixes: `rules` maps a prefix of `model.named_parameters()` names to
    group options, e.g. {"encoder.": {"frozen": True}, "decoder.": {"lr_scale": 0.5, "weight_decay": 1e-2,
    "decoupled_weight_decay": True}}.  The LONGEST matching prefix wins; parameters no prefix matches form one group with the
    `default` options; a prefix that matches no parameter raises ValueError, and so does one that loses every parameter it
    matches to longer prefixes (its group would be empty).  One group per rule, emitted in the order in
    which the groups first appear in `named_parameters()`.

    The flat layout is group-major, so rules by MODULE prefix keep it in model order, which `parallel.FlowBlockReducer`
    requires.  Rules that interleave the groups through the model (every bias, say) are fine on one GPU, but the reducer then
    raises its "order differs from the optimizer's flat layout" error."""
    rules = dict(rules or {})
    members: typing.Dict[typing.Optional[str], list] = {}
    for name, p in model.named_parameters():
        hits = [prefix for prefix in rules if name.startswith(prefix)]
        members.setdefault(max(hits, key=len) if hits else None, []).append(p)
    names = [name for name, _ in model.named_parameters()]
    unused = [prefix for prefix in rules if not any(name.startswith(prefix) for name in names)]
    if unused:
        raise ValueError(f"named_param_groups: no parameter name starts with {unused}")
    shadowed = [prefix for prefix in rules if prefix not in members]
    if shadowed:
        raise ValueError(f"named_param_groups: every parameter under {shadowed} is taken by a longer prefix of the rules")
    return [{"params": ps, **(dict(default or {}) if prefix is None else rules[prefix])} for prefix, ps in members.items()]


OptimizerType = Adam
