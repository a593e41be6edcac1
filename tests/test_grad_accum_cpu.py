"""CPU tests of gradient accumulation's host side: the data-parallel reducer's `no_sync()` over gloo (world_size 2) and the
public surface (`accum_steps`, the new C-ABI symbol).  No kernel is launched here."""
import inspect
import os
import re
import socket

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from helpers import ROOT

N_MICRO = 3


class _Toy(torch.nn.Module):
    """FlowGenerator's parameter naming scheme (encoder.*, decoder.flows.N.*) on plain CPU layers: three buckets."""

    def __init__(self):
        super().__init__()
        self.encoder = torch.nn.Sequential(torch.nn.Linear(4, 4), torch.nn.Linear(4, 4))
        self.decoder = torch.nn.Module()
        self.decoder.flows = torch.nn.ModuleList(torch.nn.Linear(4, 4) for _ in range(6))
        self.emb_g = torch.nn.Embedding(3, 4)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _value(rank, micro, index):
    """The fake gradient contribution of (rank, micro-step, parameter): small integers, so every sum and mean is exact in fp32."""
    return float((rank + 1) * (micro + 1) + index)


def _accum_worker(rank, world, port, q):
    import sys

    sys.path[:0] = [os.path.join(ROOT, "glow-tts-train_amd"), ROOT]
    from glow_tts_train import convops, optimize, parallel

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.manual_seed(3)
        model = _Toy()
        opt = optimize.Adam(model.parameters(), scheduler="noam", dim_model=4)
        red = parallel.FlowBlockReducer(model, opt)
        params = list(model.parameters())
        out = {"rank": rank, "n_buckets": len(red.buckets), "updates": []}

        def micro_step(micro):
            with torch.no_grad():
                for i, p in enumerate(params):
                    p.grad.add_(_value(rank, micro, i))
            # the operators announce a block's gradients as one list; here: the decoder first, then the rest
            dec = [p for n, p in model.named_parameters() if n.startswith("decoder.")]
            convops._notify(dec)
            convops._notify([p for p in params if all(p is not d for d in dec)])

        for _update in range(2):
            rec = {}
            opt.zero_grad()
            before = red.collectives_launched
            with red.no_sync():
                micro_step(0)
                micro_step(1)
                rec["deferred_collectives"] = red.collectives_launched - before
                rec["deferred_state"] = (len(red._seen), len(red._announced), sum(red._launched), len(red._works))
                try:
                    red.finish()
                    rec["finish_in_no_sync"] = "no error"
                except RuntimeError as exc:
                    rec["finish_in_no_sync"] = str(exc)
            rec["state_at_last"] = (len(red._seen), len(red._announced), sum(red._launched),
                                    red._pending == [b.n_params for b in red.buckets])
            micro_step(2)
            rec["launched_by_announcements"] = sum(red._launched)
            red.finish()
            rec["launched_last_update"] = red.launched_last_update
            rec["launched_in_backward"] = red.launched_in_backward
            rec["flat_g"] = opt._optim.flat_g.numpy().copy()
            out["updates"].append(rec)
        out["slices"] = opt._optim.slices()
        q.put(out)
    finally:
        dist.destroy_process_group()


def test_reducer_no_sync_defers_collectives_gloo_world2():
    """FlowBlockReducer.no_sync(): three fake micro-steps per rank (known integers added into `.grad`, then announced through
    convops._notify), the first two deferred.  No collective during the deferred ones, one per bucket for the update, and the
    reduced flat gradient is exactly the mean over ranks of each rank's three-step sum.  (FlatAdam is built on CPU tensors, as in
    the existing gloo tests.)"""
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_accum_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=120) for _ in range(world)), key=lambda r: r["rank"])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for r in res:
        nb = r["n_buckets"]
        assert nb == 3
        assert len(r["updates"]) == 2
        for rec in r["updates"]:                                  # the second update behaves exactly like the first
            assert rec["deferred_collectives"] == 0
            assert rec["deferred_state"] == (0, 0, 0, 0)
            assert "no_sync" in rec["finish_in_no_sync"]
            assert rec["state_at_last"] == (0, 0, 0, True)
            assert rec["launched_by_announcements"] == nb        # the last micro-step's announcements launch as ever
            assert rec["launched_last_update"] == nb
            assert rec["launched_in_backward"] == nb
            flat_g = torch.from_numpy(rec["flat_g"])
            for i, (o, n) in enumerate(r["slices"]):
                want = sum(_value(rk, m, i) for rk in range(world) for m in range(N_MICRO)) / world
                assert torch.equal(flat_g[o:o + n], torch.full((n,), want)), (i, flat_g[o:o + n], want)
    assert all(torch.equal(torch.from_numpy(a["flat_g"]), torch.from_numpy(b["flat_g"]))
               for a, b in zip(res[0]["updates"], res[1]["updates"]))


def test_no_sync_is_not_reentrant_and_single_process_is_quiet():
    import sys
    sys.path[:0] = [p for p in (os.path.join(ROOT, "glow-tts-train_amd"),) if p not in sys.path]
    import pytest
    from glow_tts_train import optimize, parallel

    model = _Toy()
    opt = optimize.Adam(model.parameters(), scheduler="noam", dim_model=4)
    red = parallel.FlowBlockReducer(model, opt)
    with red.no_sync():
        with pytest.raises(RuntimeError):
            with red.no_sync():
                pass
        with pytest.raises(RuntimeError, match="no_sync"):
            red.finish()
    red.finish()                                                 # outside the block: the one-process no-op it always was
    assert red.collectives_launched == 0 and red.launched_last_update == 0


def test_accum_steps_keyword_and_new_symbol():
    import pytest
    from glow_tts_train import _hip, config, train

    for fn in (train.train_step, train.train):
        p = inspect.signature(fn).parameters["accum_steps"]
        assert p.default == 1
    sig = inspect.signature(train.train_batches)
    assert list(sig.parameters)[:5] == ["model", "optimizer", "batches", "grad_clip", "reducer"]
    assert sig.parameters["reducer"].default is None
    assert "accum_steps" not in config.TrainingConfig.__dataclass_fields__   # the config's JSON surface is the reference's
    name = "glowtts_clip_grad_value_scaled"
    assert name in _hip.EXPORTED_SYMBOLS and name in _hip._SIGNATURES
    header = open(os.path.join(ROOT, "include", "glowtts_hip.h")).read()
    assert re.search(r"\bint\s+" + name + r"\s*\(\s*float \*g, int64_t n, float scale, float clip, float \*sumsq", header)
    assert inspect.signature(__import__("glow_tts_train.optimize", fromlist=["x"]).FlatAdam.clip_grad_value_).parameters["scale"].default == 1.0
    # wrong arguments are refused before any batch is touched
    with pytest.raises(ValueError, match="accum_steps"):
        train.train_step(1, 1, torch.nn.Linear(1, 1), None, None, [], accum_steps=0)
    with pytest.raises(ValueError, match="GradScaler"):
        train.train_step(1, 1, torch.nn.Linear(1, 1), None, None, [], scaler=object(), accum_steps=2)


def test_weights_scope_bookkeeping():
    """convops.weights_unchanged(): not re-entrant, ended by an exception, and the optimizer refuses to step inside it."""
    import pytest
    from glow_tts_train import _hip, convops, optimize

    ws = _hip.weights_state
    e0 = ws.epoch
    convops.weights_changed(record=True)
    assert ws.epoch == e0 + 1 and ws.record and not ws.active
    opt = optimize.FlatAdam([torch.nn.Parameter(torch.zeros(3))])
    with pytest.raises(ZeroDivisionError):
        with convops.weights_unchanged():
            assert ws.active
            with pytest.raises(RuntimeError):
                with convops.weights_unchanged():
                    pass
            with pytest.raises(RuntimeError, match="weights_unchanged"):
                opt.step()
            ws.loose["x"] = 1
            1 / 0
    assert not ws.active and not ws.record and not ws.loose
