#!/usr/bin/env python3
"""Every native call the stacked decoder / encoder nodes of convops.py queue in one forward + backward, in a form that can
be compared between two trees with `diff`: entry point, stream, scalars, and each pointer as (allocation, byte offset).

`convops.call` and `_hip.call_on` are wrapped as convops sees them, `convops.ptr` too: the tensors that pass through it name the
allocations (their storage's base and size), numbered by first appearance in a traced call; the tool keeps them alive until the
pass ends, or the numbering would depend on when the caching allocator gets memory back from the second stream.  A pointer outside all of them (a
packed weight, a bias: addresses the cached tables hold) is numbered by first appearance as `ext`; a table argument is printed
as the block / layer it belongs to.  One untraced pass runs first, so that the caches the nodes keep are filled.

    python tools/flow_call_trace.py [config ...] > trace.txt          (no argument: all configurations)
"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "glow-tts-train_amd")]
import torch  # noqa: E402

from glow_tts_train import _hip, attentions, convops, models  # noqa: E402

DEV = "cuda"
PTR, CALL, CALL_ON = convops.ptr, convops.call, _hip.call_on


class Trace:
    def __init__(self):
        self.storages = []            # (base, bytes) of the tensors that passed through convops.ptr, the latest last
        self.alive = []               # ... and the tensors: nothing they own is freed and handed out again during the traced pass
        self.allocs, self.ext, self.streams, self.tables = {}, {}, {}, {}
        self.lines, self.on = [], False

    # -- the three wrapped functions
    def ptr(self, t):
        if t is not None and self.on:
            st = t.untyped_storage()
            key = (st.data_ptr(), st.nbytes())
            if key in self.storages:
                self.storages.remove(key)
            self.storages.append(key)
            self.alive.append(t)
        return PTR(t)

    def call(self, name, *args, **kw):
        if self.on:
            cur = torch.cuda.current_stream().cuda_stream
            self.lines.append(f"{name} current({self.stream(cur)}) " + " ".join(self.arg(a) for a in args))
        return CALL(name, *args, **kw)

    def call_on(self, stream_ptr, name, *args):
        if self.on:
            self.lines.append(f"{name} explicit({self.stream(stream_ptr)}) " + " ".join(self.arg(a) for a in args))
        return CALL_ON(stream_ptr, name, *args)

    # -- how an argument is printed
    def stream(self, handle):
        return self.streams.setdefault(handle, "s%d" % len(self.streams))

    def arg(self, a):
        if a is None:
            return "null"
        if isinstance(a, float):
            return repr(a)
        if not isinstance(a, int) or isinstance(a, bool) or abs(a) < (1 << 32):
            return str(int(a))
        if a in self.tables:
            return self.tables[a]
        if a in self.streams or a in [s.cuda_stream for s in _hip._side_streams.values()]:
            return "stream(%s)" % self.stream(a)
        for base, size in reversed(self.storages):
            if base <= a < base + size:
                n = self.allocs.setdefault((base, size), len(self.allocs))
                return f"(a{n}:{size},{a - base})"
        return "ext%d" % self.ext.setdefault(a, len(self.ext))


def flow_case(h, blocks, gin, io, switches):
    torch.manual_seed(77)
    b, t = 2, 40                                          # t: frames after the squeeze
    dec = models.FlowSpecDecoder(80, h, kernel_size=5, dilation_rate=1, n_blocks=blocks, n_layers=3, p_dropout=0.05, n_split=4,
                                 n_sqz=2, sigmoid_scale=False, gin_channels=gin).to(DEV).train()
    for p in dec.parameters():
        p.grad = torch.zeros_like(p)
    g = torch.randn(b, gin, 1, device=DEV) if gin else None
    y0 = torch.randn(b, 80, 2 * t, device=DEV)
    lens = torch.tensor([2 * t, 2 * t - 10], device=DEV)
    mask = (torch.arange(2 * t, device=DEV)[None] < lens[:, None]).float().unsqueeze(1)

    def step():
        saved = {k: getattr(convops, k) for k in switches}
        dec.io_bf16 = io
        try:
            for k, v in switches.items():
                setattr(convops, k, v)
            with _hip.zero_scope(y0.device):              # a training step: the weight-gradient stream is in use
                z, ld = dec((y0 * mask).clone().requires_grad_(True), mask, g=g)
                (z.sum() + ld.sum()).backward()
                _hip.join_side_streams()
                convops.flush_groups()
            torch.cuda.synchronize()
        finally:
            for k, v in saved.items():
                setattr(convops, k, v)

    def tables():
        plans = [f._block_plan for f in dec.flows if hasattr(f, "_block_plan")]
        return {ctypes.addressof(p._tab): "block%d" % i for i, p in enumerate(plans)}
    return step, tables


def encoder_case(stack):
    torch.manual_seed(13)
    b, h, t, nl = 2, 32, 16, 2
    enc = attentions.Encoder(h, 64, 2, nl, kernel_size=3, p_dropout=0.1, window_size=4).to(DEV).train()
    groups = [convops.ConvGroup([a.conv_q, a.conv_k, a.conv_v, a.conv_o, f.conv_1, f.conv_2])
              for a, f in zip(enc.attn_layers, enc.ffn_layers)]
    for p in enc.parameters():
        p.grad = torch.zeros_like(p)
    x0 = torch.randn(b, h, t, device=DEV)
    lens = torch.tensor([t, t - 5], device=DEV)
    mask = (torch.arange(t, device=DEV)[None] < lens[:, None]).float().unsqueeze(1)

    def step():
        before, attentions._ENC_STACK = attentions._ENC_STACK, stack
        try:
            with _hip.zero_scope(x0.device):
                for g in groups:
                    g.begin()
                enc(x0.clone().requires_grad_(True), mask).sum().backward()
                _hip.join_side_streams()
                convops.flush_groups()
            torch.cuda.synchronize()
        finally:
            attentions._ENC_STACK = before

    def tables():
        return {ctypes.addressof(g._enc_tab): "layer%d" % i for i, g in enumerate(groups)}
    return step, tables


# the bf16-tensor kernels exist at the default coupling width only (flow_block_bf16_ok): that configuration runs with H = 192
CONFIGS = {
    "flow-stack-chains": lambda: flow_case(48, 3, 0, False, {"_HALF_BATCH_FWD": True}),
    "flow-stack-one-chain": lambda: flow_case(48, 3, 0, False, {"_HALF_BATCH_FWD": False}),
    "flow-stack-boundary-bwd": lambda: flow_case(48, 3, 0, False, {"_HALF_BATCH_FWD": True, "_FLOW_BOUNDARY_BWD": True}),
    "flow-stack-io1": lambda: flow_case(192, 3, 0, "hidden", {}),
    "flow-per-block-gin8": lambda: flow_case(48, 3, 8, False, {}),
    "encoder-stack": lambda: encoder_case(True),
    "encoder-per-layer": lambda: encoder_case(False),
}


def main():
    names = sys.argv[1:] or list(CONFIGS)
    _hip.load()
    for name in names:
        step, tables = CONFIGS[name]()
        step()                                            # fills the nodes' caches (tables, plans, the allocator's pools)
        tr = Trace()
        tr.tables = tables()
        convops.ptr, convops.call, _hip.call_on = tr.ptr, tr.call, tr.call_on
        tr.on = True
        try:
            step()
        finally:
            tr.on = False
            convops.ptr, convops.call, _hip.call_on = PTR, CALL, CALL_ON
        print(f"== {name}: {len(tr.lines)} calls")
        for line in tr.lines:
            print(line)


if __name__ == "__main__":
    main()
