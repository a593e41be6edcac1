"""ctypes binding of libglowtts_hip.so (include/glowtts_hip.h) — the only way the Python host reaches the GPU kernels.

PyTorch is used for device memory (``tensor.data_ptr()``) and streams (``torch.cuda.current_stream()``); the
kernels themselves are the hand-written HIP in ``glow-tts-train_amd/csrc``.  There is NO fallback: if the library
is missing, or a tensor handed to an operator is not a contiguous fp32 CUDA/HIP tensor, the call raises.

Prototypes, structs and flag constants are read from the header at import (``_cabi.py``): a new entry point is declared
in ``include/glowtts_hip.h`` and nowhere else.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional

import torch

from . import _cabi
from ._cabi import HipLibraryMissing  # noqa: F401  (raised by load(), caught by importers)

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.environ.get(
    "GLOWTTS_HIP_LIB", os.path.join(os.path.dirname(_PKG_DIR), "lib", "libglowtts_hip.so")
)

# Everything below is DERIVED from the header the library is compiled against (_cabi.py): to add an entry point, declare it
# in include/glowtts_hip.h — there is no table to extend here.
_FUNCTIONS, _STRUCTS, CONSTANTS = _cabi.read_header()

# name -> argument ctypes of every function that returns int and ends in a glowtts_stream_t (`call` appends the stream;
# glowtts_wn_bwd's wgrad_stream is an ordinary argument)
_SIGNATURES = {name: args[:-1] for name, (_, args, streamed) in _FUNCTIONS.items() if streamed}

# HOST structs of device pointers handed to the multi-launch executors (fields and their order are the header's)
WnLayer = _STRUCTS["glowtts_wn_layer"]
Wrw1Problem = _STRUCTS["glowtts_wrw1_problem"]
FlowBlock = _STRUCTS["glowtts_flow_block"]
EncLayer = _STRUCTS["glowtts_enc_layer"]
ConvPlan = _STRUCTS["glowtts_conv_plan"]          # written BY the library: glowtts_conv_plan_next
AttnPlan = _STRUCTS["glowtts_attn_plan"]          # ... glowtts_attn_plan_for
FlowPlan = _STRUCTS["glowtts_flow_plan"]          # ... glowtts_flow_plan_for
WnBwdPlan = _STRUCTS["glowtts_wn_bwd_plan"]       # ... glowtts_wn_bwd_plan_for

EXPORTED_SYMBOLS = sorted(_FUNCTIONS)

_I = ctypes.c_int

_lib: Optional[ctypes.CDLL] = None
_fn_cache: dict = {}


def library_path() -> str:
    return _LIB_PATH


def load() -> ctypes.CDLL:
    """Load (once) and type the C-ABI library.  Raises HipLibraryMissing — never falls back to another path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise HipLibraryMissing(
            f"{_LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  This package has no CPU or eager fallback."
        )
    lib = ctypes.CDLL(_LIB_PATH)
    for name, (restype, args, _) in _FUNCTIONS.items():
        fn = getattr(lib, name)
        fn.restype = restype
        fn.argtypes = list(args)
    _lib = lib
    _bind_fastcall(lib)
    return lib


def _bind_fastcall(lib) -> None:
    """`call()` goes through `_glowtts_fastcall` when it is there (csrc/gen_fastcall.py: METH_FASTCALL wrappers around the
    same entry points, ~3 us less host time per call than ctypes' argument conversion, ~1 000 calls per step).  It is
    only a binding: its function pointers are taken from the ctypes handle opened above, and without it every call goes
    through ctypes.  GLOWTTS_FASTCALL=0 disables it."""
    global FASTCALL
    FASTCALL = False
    if os.environ.get("GLOWTTS_FASTCALL", "1") == "0":
        return
    lib_dir = os.path.join(os.path.dirname(_PKG_DIR), "lib")
    try:
        import importlib.machinery
        import importlib.util
        import sysconfig

        path = os.path.join(lib_dir, "_glowtts_fastcall" + sysconfig.get_config_var("EXT_SUFFIX"))
        if not os.path.exists(path):
            return
        loader = importlib.machinery.ExtensionFileLoader("_glowtts_fastcall", path)
        mod = importlib.util.module_from_spec(importlib.util.spec_from_loader("_glowtts_fastcall", loader))
        loader.exec_module(mod)
        if sorted(mod.NAMES) != sorted(_SIGNATURES):          # built from another _hip.py: ignore it
            return
        for i, name in enumerate(mod.NAMES):
            mod._bind(i, ctypes.cast(getattr(lib, name), ctypes.c_void_p).value)
        for name in mod.NAMES:
            _fn_cache[name] = getattr(mod, name)
        FASTCALL = True
    except Exception:                                         # a binding convenience must never stop the library loading
        _fn_cache.clear()


FASTCALL = False


def direct_apply(cls):
    """`cls.apply` without the Python wrapper of torch.autograd.Function.apply (default-argument binding for setup_context
    and functorch unwrapping, neither used by these operators): the engine's own entry point, ~4 us less per call on a path
    that makes ~130 such calls per step and is within 20 % of being host-bound."""
    return super(torch.autograd.Function, cls).apply


CONV_MATH_MODES = {"fp32": 0, "bf16": 1, "bf16x3": 2, "bf16x6": 3}


def conv_math(mode=None) -> int:
    """Arithmetic of the WN convolutions (include/glowtts_hip.h: glowtts_conv_math): "fp32" (native MFMA, default),
    "bf16", "bf16x3", "bf16x6" or the numeric code; None only queries.  Returns the mode in force BEFORE the call."""
    lib = load()
    before = lib.glowtts_conv_math(-1)
    if mode is not None:
        if isinstance(mode, str):            # "bf16x6" or "bf16x6+wrw" (the weight-gradient kernel as well)
            base, _, wrw = mode.partition("+")
            if base not in CONV_MATH_MODES or wrw not in ("", "wrw"):
                raise ValueError(f"conv math mode {mode!r}: expected one of {sorted(CONV_MATH_MODES)}, optionally with '+wrw'")
            code = CONV_MATH_MODES[base] * (5 if wrw == "wrw" else 1)
        else:
            code = int(mode)
        if lib.glowtts_conv_math(code) != 0:
            raise RuntimeError(lib.glowtts_last_error().decode())
    return before


def wn_fused(enable: Optional[bool] = None) -> bool:
    """The layer-resident WN forward kernel (include/glowtts_hip.h: glowtts_wn_fused): True / False switches it, None only
    queries.  Returns the setting in force BEFORE the call."""
    return bool(load().glowtts_wn_fused(-1 if enable is None else int(bool(enable))))


def wn_fused_launches() -> int:
    """Launches of the layer-resident WN forward kernel so far in this process."""
    return int(load().glowtts_wn_fused(-2))


def set_knob(name: str, value: int) -> None:
    """Set one of the library's tuning switches (include/glowtts_hip.h, conventions block) for the launches queued from now
    on; an unknown name raises."""
    lib = load()
    if lib.glowtts_set_knob(name.encode(), int(value)) != 0:
        raise RuntimeError(lib.glowtts_last_error().decode())


def get_knob(name: str) -> int:
    lib = load()
    out = _I(0)
    if lib.glowtts_get_knob(name.encode(), ctypes.byref(out)) != 0:
        raise RuntimeError(lib.glowtts_last_error().decode())
    return int(out.value)


def conv_bind_planes(wp: Optional[torch.Tensor], planes: Optional[torch.Tensor] = None):
    """Bind (or, with None, unbind) a packed-weight buffer's bf16 planes for this thread's next convolution launches."""
    lib = load()
    if wp is None:
        lib.glowtts_conv_bind_planes(None, 0, None)
    elif lib.glowtts_conv_bind_planes(wp.data_ptr(), wp.numel(), planes.data_ptr()) != 0:
        raise RuntimeError(lib.glowtts_last_error().decode())


def wino_launches() -> int:
    """Launches of the Winograd form of the gated in-conv (csrc/convwino.hip) by this process so far."""
    return int(load().glowtts_wino_launches())


def wino_bwd_launches() -> int:
    """Launches of the Winograd form of the gated in-conv's backward-data (csrc/convwino.hip) by this process so far."""
    return int(load().glowtts_wino_bwd_launches())


def wino_plane_elems(n: int) -> int:
    """bf16 elements per plane of the Winograd-domain weights (csrc/convwino.hip) of a packed buffer of `n` floats."""
    return int(load().glowtts_wino_plane_elems(int(n)))


def conv_bind_wino(wp: Optional[torch.Tensor], planes: Optional[torch.Tensor] = None):
    """Bind (None: unbind) the Winograd-domain planes (3 x wino_plane_elems(n) bf16, written by glowtts_wino_weights) of a packed-weight
    buffer for this thread's next gated in-conv launches (used when the switch GLOWTTS_WINO is on)."""
    lib = load()
    if wp is None:
        lib.glowtts_conv_bind_wino(None, 0, None, 0)
    elif lib.glowtts_conv_bind_wino(wp.data_ptr(), wp.numel(), planes.data_ptr(), planes.numel() // 3) != 0:
        raise RuntimeError(lib.glowtts_last_error().decode())


def conv_bind_planes_ns(wp: Optional[torch.Tensor], planes: Optional[torch.Tensor] = None, n_planes: int = 1):
    """Bind (None: unbind) `n_planes` bf16 planes of a packed-weight buffer for this thread's next convolution launches,
    whatever glowtts_conv_math says (bf16-tensor flow blocks bind ONE plane: the weights rounded to bf16)."""
    lib = load()
    if wp is None:
        lib.glowtts_conv_bind_planes_ns(None, 0, None, 0)
    elif lib.glowtts_conv_bind_planes_ns(wp.data_ptr(), wp.numel(), planes.data_ptr(), int(n_planes)) != 0:
        raise RuntimeError(lib.glowtts_last_error().decode())


def ptr(t: Optional[torch.Tensor]):
    """Device pointer of a contiguous CUDA/HIP tensor (None -> NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError(
            "glow_tts_train (MI355X build): operator received a CPU tensor; this package runs only on HIP devices"
        )
    if not t.is_contiguous():
        raise RuntimeError("glow_tts_train: non-contiguous tensor passed to a HIP kernel")
    return t.data_ptr()


def f32(t: torch.Tensor) -> torch.Tensor:
    if t.dtype != torch.float32:
        raise RuntimeError(f"glow_tts_train: HIP kernels are fp32, got {t.dtype}")
    return t


# Optional per-kernel timing with HIP events recorded on the launch stream (bench.py's roofline leg).  Off by
# default: the product path records nothing.
_timing: Optional[dict] = None


def enable_timing() -> None:
    global _timing
    _timing = {}


def disable_timing() -> dict:
    """Stop timing and return {name: [milliseconds per launch, ...]} (synchronises once to read the events)."""
    global _timing
    t, _timing = _timing or {}, None
    torch.cuda.synchronize()
    return {k: [a.elapsed_time(b) for a, b in v] for k, v in t.items()}


_side_streams: dict = {}


def side_stream_enabled() -> bool:
    """The text encoder may run on a second stream next to the flow decoder (models.FlowGenerator.forward), but only
    inside a training step bracketed by `zero_scope` (train.train_batch joins the stream again after backward — gradients
    the operators write straight into `.grad` never pass an AccumulateGrad node, so autograd's own end-of-backward stream
    sync does not cover them).  Off while per-launch timings are collected (overlapped kernels would time each other)
    and when GLOWTTS_SIDE_STREAM=0."""
    return _arena.active and _timing is None and os.environ.get("GLOWTTS_SIDE_STREAM", "1") != "0"


def timing_off() -> bool:
    """False while per-launch timings are collected: multi-launch native executors then yield to the per-kernel path."""
    return _timing is None


def join_side_streams() -> None:
    """Make the current stream wait for everything queued on the side streams (after backward, before the optimizer)."""
    for (_, role), s in _side_streams.items():
        if not role.startswith("fwd"):
            torch.cuda.current_stream(s.device).wait_stream(s)


def side_stream(device, role: str = "encoder", priority: int = 0) -> "torch.cuda.Stream":
    """One extra stream per (device, role): "encoder" (the text-encoder branch), "wgrad" (weight-gradient kernels) and
    "comm" (the DP reducer's collectives)."""
    if role == "fwd2" and _FWD2_ON_WGRAD:            # the decoder's second forward chain runs on the stream the weight gradients use
        role = "wgrad"                               # in the backward (idle during the forward): one stream fewer — DESIGN.md lesson 38
    key = (torch.device(device).index, role)
    if key not in _side_streams:
        _side_streams[key] = torch.cuda.Stream(device, priority=priority)
    return _side_streams[key]


_FWD2_ON_WGRAD = os.environ.get("GLOWTTS_FWD2_ON_WGRAD", "1") != "0"


def all_side_streams(device):
    """The side streams gradients may come from (the forward-only chains "fwd2.." are joined inside the forward: not among them)."""
    idx = torch.device(device).index
    return [s for (d, role), s in _side_streams.items() if d == idx and not role.startswith("fwd")]


def call(name: str, *args, tag=None) -> None:
    """Launch `name` on PyTorch's current stream; raise RuntimeError with the library's message on failure.
    `tag` only labels the launch for the optional timing table: a string, or a (format, *values) tuple that is formatted
    only when timings are being collected.  This function runs ~1 100 times per training step, so the untimed path does
    nothing but look up the cached ctypes entry and the raw stream handle."""
    fn = _fn_cache.get(name)
    if fn is None:
        fn = _fn_cache[name] = getattr(load(), name)
    if _timing is None:
        rc = fn(*args, torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice()))
    else:
        cur = torch.cuda.current_stream()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(cur)
        rc = fn(*args, cur.cuda_stream)
        b.record(cur)
        if isinstance(tag, tuple):
            tag = tag[0] % tag[1:]
        _timing.setdefault(name if tag is None else f"{name}[{tag}]", []).append((a, b))
    if rc != 0:
        msg = load().glowtts_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"{name} failed (code {rc}): {msg}")


def call_on(stream_ptr: int, name: str, *args) -> None:
    """`call` on an explicit raw HIP stream (no stream context switch on the host: the stack node's two forward chains)."""
    fn = _fn_cache.get(name)
    if fn is None:
        fn = _fn_cache[name] = getattr(load(), name)
    rc = fn(*args, stream_ptr)
    if rc != 0:
        msg = load().glowtts_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"{name} failed (code {rc}): {msg}")


# ----------------------------------------------------------------------------------------------------------------
class _ZeroArena:
    """Zero-initialised scratch for ONE training step: accumulators the kernels add into with atomics (packed weight
    gradients, log-determinants, loss sums) are carved out of one buffer that a step clears with ONE fill instead of
    ~100 `torch.zeros` launches.  Only temporaries that die inside the step live here — never a tensor handed to
    autograd as a parameter gradient (AccumulateGrad may keep such a tensor as `param.grad`)."""

    def __init__(self):
        self.buf: Optional[torch.Tensor] = None
        self.off = 0          # floats handed out in the current step
        self.want = 0         # floats requested in the current step (sizes the buffer of the next one)
        self.active = False

    def begin(self, device) -> None:
        if self.want and (self.buf is None or self.buf.device != torch.device(device) or self.want > self.buf.numel()):
            if not torch.cuda.is_current_stream_capturing():
                self.buf = torch.empty(int(self.want * 1.25) + 1024, device=device, dtype=torch.float32)
        if self.buf is not None:
            self.buf.zero_()
        self.off, self.want, self.active = 0, 0, True

    def end(self) -> None:
        self.active = False

    def zeros(self, shape, device) -> torch.Tensor:
        n = 1
        for d in shape:
            n *= int(d)
        span = (n + 63) // 64 * 64                      # 256-byte granules keep every carve-out 16-byte aligned
        if self.active:
            self.want += span
            if self.buf is not None and self.buf.device == torch.device(device) and self.off + span <= self.buf.numel():
                out = self.buf[self.off: self.off + n].view(shape)
                self.off += span
                return out
        return torch.zeros(shape, device=device, dtype=torch.float32)


_arena = _ZeroArena()


class zero_scope:
    """`with zero_scope(device):` brackets one training step (train.train_batch); inside it `scratch_zeros` carves from
    the arena, outside it is plain `torch.zeros`."""

    def __init__(self, device):
        self.device = device

    def __enter__(self):
        _arena.begin(self.device)
        return self

    def __exit__(self, *exc):
        _arena.end()
        return False


def scratch_zeros(shape, device) -> torch.Tensor:
    return _arena.zeros(tuple(shape) if not isinstance(shape, int) else (shape,), device)


class _WeightsState:
    """State of `convops.weights_unchanged()` (gradient accumulation: the weights do not change between the micro-batches of
    one update, so what is derived from them alone is made once per update).  It lives here because the operators of ops.py,
    convops.py and the optimizer all read it.
      active — inside the scope: a request for weight-derived data may be answered with what the same `epoch` already made;
      epoch  — counts the times the weights may have changed (`convops.weights_changed()`); everything derived from the weights
               remembers the epoch it was made in, and only data of the CURRENT epoch is ever reused;
      record — loose results (a single convolution's packed weights, one flow's W^-1) are kept in `loose` for the scope to find;
               off outside an accumulated update, so that nothing outlives the step that made it on the ordinary path."""

    def __init__(self):
        self.active, self.epoch, self.record = False, 0, False
        self.loose: dict = {}


weights_state = _WeightsState()
