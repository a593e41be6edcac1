"""glowtts_conv_wrw1_multi (csrc/convwrw1.hip, convwrw1_kernel) through the C ABI (glow_tts_train._hip.call) against plain fp64 torch
on the CPU: the 1x1 weight gradients of several problems of DIFFERENT shapes in one launch,

    dwp[k][m] += sum_{b,t} x[b][k][t] (* mask_x[b][t]) * d[b][m][t] (* mask_d[b][t]),      dbias[m] += sum_{b,t} d[b][m][t] (* mask_d)

with rows [d_split, M) of d from a second tensor where d2 is given (include/glowtts_hip.h).  In "bf16x6+wrw" (mode 15) the problems
of a dispatch (at most 8) share one launch whose split-K count is (GLOWTTS_WRW1_CUS / tiles), whatever the shape; in native
arithmetic (mode 0), with GLOWTTS_WRW1_MULTI = 0 and for shapes outside the kernel's (T % 4, x_bs % 4, a misaligned mask) the entry
launches the problems one by one: "same results either way".  tests/test_conv_math.py compares max|err| / max|ref| per problem on
random data with the split count that 15 tiles happen to get on the chip at hand.  The GPU tests are marked `gpu`; the tests at the
end of the module are not: they pin the split regimes of the rows and the bound on the CPU.

Every launch (tests/helpers.py: Dev): each input is a copy inside a guarded buffer and must be bit-identical afterwards; dwp and
dbias live between guard sentinels that must survive and start from 0 — at the row "start" from a running sum of small integers.
A channel slice (x of problem "slice": the first 80 of 160 channels) and a strided d are embedded in tensors of random values.
From two utterances on, one is empty under the masks; inputs beyond an utterance's end hold random finite values.

Two kinds of input (as tests/test_conv_kernels.py):
  1. Counting: x, d integers in [-2, 2], masks 0 / 1.  The sum of absolute terms is asserted below 2**24 per problem, so every
     partial sum is exact in fp32 in any order and in any split: ALL outputs are asserted EQUAL to fp64, in both modes (a small
     integer is its own bf16 plane 0).
  2. Random: x, d ~ N(0, 1).  Per element |got - want| <= 1e-5 sum|term|, the project's figure for "block sum + float atomics"
     (tests/test_conv_kernels.py, tests/test_flow_kernels.py); fp32 torch on the CPU shows at most 3.3e-7 of sum|term| on these
     inputs (test_fp32_cpu_share_of_the_reduction_bound; printed beside every GPU figure), the MI355X at most 1.6e-7 in
     either mode (profiles/r17_wino_wrw1_kernels.txt).

Problems (Cin, M, d_split): PROBLEMS below — 1 x 1, 16 x 16, the 192 / 128 tile edges from below, exactly and from above, the two
two-source shapes of a flow block, both masks with an empty utterance, a slice and a strided d, and one without dbias.  LISTS: all nine
table problems (two dispatches: 8 + 1), exactly eight, and single problems.  (B, T): (1, 4), (2, 32), (3, 36) (a 4-frame last step)
and (2, 64).  Split regimes, selected with GLOWTTS_WRW1_CUS so that they do not depend on the chip: splits = 1; splits = total steps
(nb = 1); 16 splits over 18 steps (nb = 2: splits 9 .. 15 are empty) with GLOWTTS_WRW1_XCD 1 and 0; 20 compute units over 18 steps
(XCD 1: rounded down to 16 splits, the empty form; XCD 0: 18 splits of one step).  _dispatch_mirror restates conv_wrw1_multi_dispatch
and test_rows_reach_their_split_regimes asserts every row's regime on the CPU.
"""
import ctypes
import functools
import types

import pytest
import torch

from helpers import Dev, GUARD

gpu = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
RED_BOUND = 1e-5         # of sum|term|: the project's figure for a block sum plus float atomics
MODES = (15, 0)
TK, TM, STEP, MAX_BATCH = 192, 128, 32, 8          # the kernel's tile (x channels, d channels), frames per step, problems per dispatch


def _p(name, Cin, M, d_split=0, mask_d=False, mask_x=False, x_slice=False, d_strided=False, dbias=True):
    return types.SimpleNamespace(name=name, Cin=Cin, M=M, d_split=d_split, mask_d=mask_d, mask_x=mask_x, x_slice=x_slice,
                                 d_strided=d_strided, dbias=dbias)


PROBLEMS = [_p("1x1", 1, 1), _p("16x16", 16, 16), _p("191x127", 191, 127), _p("192x128", 192, 128), _p("193x129", 193, 129),
            _p("two-384", 192, 384, 192), _p("two-320", 64, 320, 64), _p("masks", 200, 200, mask_d=True, mask_x=True),
            _p("slice", 80, 192, x_slice=True, d_strided=True), _p("nobias", 48, 16, dbias=False)]
_BY_NAME = {p.name: p for p in PROBLEMS}
LISTS = {"nine": [p.name for p in PROBLEMS[:9]],
         "eight": [p.name for p in PROBLEMS[:7]] + ["nobias"],
         "single": ["16x16"],
         "one-source": ["1x1", "16x16", "191x127", "193x129", "masks", "slice", "nobias"]}


def _row(name, why, probs, B, T, cus, regime, xcd=1, multi=1, odd_x_bs=False, mis_mask=False, start=False):
    return types.SimpleNamespace(name=name, why=why, probs=probs, B=B, T=T, cus=cus, regime=regime, xcd=xcd, multi=multi,
                                 odd_x_bs=odd_x_bs, mis_mask=mis_mask, start=start)


# regime: "one" (splits = 1), "steps" (splits = total steps, nb = 1), "empty" (>= 16 splits, a multiple of 8, some without a step),
# "fallback" (mode 15 launches the problems one by one as well)
ROWS = [
    _row("nine-B1T4-one", "one 4-frame step in all; nine problems = two dispatches", "nine", 1, 4, 1, "one"),
    _row("nine-B2T32-one", "two whole steps in ONE workgroup per tile: both wave groups work", "nine", 2, 32, 1, "one"),
    _row("nine-B2T32-steps", "one step per split", "nine", 2, 32, 2 * 20, "steps"),
    _row("nine-B3T36-one", "a 4-frame last step per utterance; six steps in one workgroup", "nine", 3, 36, 1, "one"),
    _row("nine-B3T36-steps", "every split is one step: full and 4-frame steps apart", "nine", 3, 36, 6 * 20, "steps", start=True),
    _row("eight-B2T64-steps", "exactly eight problems: one dispatch; four steps, four splits", "eight", 2, 64, 4 * 20, "steps"),
    _row("eight-B3T36-one", "exactly eight problems, one split", "eight", 3, 36, 19, "one"),
    _row("single-B3T164-empty", "16 splits of 2 steps over 18 steps: splits 9 .. 15 are empty", "single", 3, 164, 16, "empty"),
    _row("single-B3T164-empty-noxcd", "the same with GLOWTTS_WRW1_XCD = 0", "single", 3, 164, 16, "empty", xcd=0),
    _row("single-B3T164-cus20", "20 compute units: rounded down to 16 splits", "single", 3, 164, 20, "empty"),
    _row("single-B3T164-cus20-noxcd", "20 compute units, not rounded: 18 splits of one step", "single", 3, 164, 20, "steps", xcd=0),
    _row("fb-T38", "T % 4 != 0: one by one", "one-source", 3, 38, 40, "fallback"),
    _row("fb-xbs", "x_bs % 4 != 0: one by one", "one-source", 3, 36, 40, "fallback", odd_x_bs=True),
    _row("fb-mask", "the mask one float off a 16-byte boundary: one by one", "one-source", 3, 36, 40, "fallback", mis_mask=True),
    _row("fb-multi0", "GLOWTTS_WRW1_MULTI = 0: one by one", "nine", 3, 36, 40, "fallback", multi=0),
]
ROW_PARAMS = [pytest.param(r, id=r.name) for r in ROWS]


def _dispatch_mirror(probs, B, T, cus, xcd):
    """(splits, nb, total steps, tiles) of conv_wrw1_multi_dispatch (csrc/convwrw1.hip) for one dispatch of <= 8 problems with
    GLOWTTS_WRW1_CUS = cus > 0."""
    assert 1 <= len(probs) <= MAX_BATCH and cus > 0
    tiles = sum(-(-p.Cin // TK) * -(-p.M // TM) for p in probs)
    total = B * -(-T // STEP)
    splits = cus // tiles
    if splits >= 16 and xcd:
        splits &= ~7
    splits = max(1, min(splits, total))
    nb = -(-total // splits)
    if not (splits >= 16 and splits % 8 == 0):
        splits = -(-total // nb)
    return splits, nb, total, tiles


def _row_regimes(row):
    """The regime of every dispatch of the row in mode 15."""
    probs = [_BY_NAME[n] for n in LISTS[row.probs]]
    one_by_one = row.multi == 0 or row.T % 4 != 0 or row.T < 4 or row.odd_x_bs or (row.mis_mask and any(p.mask_d or p.mask_x for p in probs))
    out = []
    for q0 in range(0, len(probs), MAX_BATCH):
        if one_by_one:
            out.append("fallback")
            continue
        splits, nb, total, _tiles = _dispatch_mirror(probs[q0: q0 + MAX_BATCH], row.B, row.T, row.cus, row.xcd)
        assert (splits - 1) * nb < total or (splits >= 16 and splits % 8 == 0), "an empty split outside the form that allows one"
        if splits >= 16 and splits % 8 == 0 and (splits - 1) * nb >= total:
            out.append("empty")
        elif splits == 1:
            out.append("one")
        elif nb == 1 and splits == total:
            out.append("steps")
        else:
            out.append(f"other:{splits}x{nb}")
    return out


# =============================================================================================== inputs and the reference
def _lengths(B, T):
    return torch.tensor([T, 0, T - 3][:B])


@functools.lru_cache(maxsize=None)
def _inputs(pname, kind, B, T):
    """The tensors of one problem, fp32 on the CPU (shared by the rows, never modified)."""
    p = _BY_NAME[pname]
    gen = torch.Generator().manual_seed(7919 * p.Cin + 104729 * p.M + 31 * B + T + 7 * len(kind))
    r = (lambda *s: torch.randint(-2, 3, s, generator=gen).float()) if kind == "count" else (lambda *s: torch.randn(*s, generator=gen))
    I = types.SimpleNamespace()
    I.xw = r(B, 160 if p.x_slice else p.Cin, T)                       # the tensor x is a channel slice of
    I.x = I.xw[:, :p.Cin]
    rows1 = p.d_split if p.d_split else p.M
    I.d, I.d2 = r(B, rows1, T), (r(B, p.M - p.d_split, T) if p.d_split else None)
    I.gap = r(B, 8)                                                     # what lies between the utterances of a strided d
    I.mask = (torch.arange(T)[None] < _lengths(B, T)[:, None]).float()
    return I


def _ref(p, I, dt):
    """name -> (value, sum of |terms|) in dtype dt, starting from 0."""
    x, d = I.x.to(dt), (torch.cat([I.d, I.d2], 1) if p.d_split else I.d).to(dt)
    if p.mask_x:
        x = x * I.mask.to(dt)[:, None]
    if p.mask_d:
        d = d * I.mask.to(dt)[:, None]
    out = {"dwp": (torch.einsum("bkt,bmt->km", x, d), torch.einsum("bkt,bmt->km", x.abs(), d.abs()))}
    if p.dbias:
        out["dbias"] = (d.sum((0, 2)), d.abs().sum((0, 2)))
    return out


def _start(numel, seed):
    return torch.randint(1, 4, (numel,), generator=torch.Generator().manual_seed(numel * 31 + seed)).float()


# =============================================================================================== the launches
@pytest.fixture()
def G():
    """The library; restores the arithmetic mode and the three switches afterwards."""
    from glow_tts_train import _hip

    lib = _hip.load()
    before = lib.glowtts_conv_math(-1)
    knobs = {k: _hip.get_knob(k) for k in ("WRW1_CUS", "WRW1_XCD", "WRW1_MULTI")}
    yield types.SimpleNamespace(hip=_hip, lib=lib)
    for k, v in knobs.items():
        _hip.set_knob(k, v)
    assert lib.glowtts_conv_math(before) == 0


def _launch(G, row, kind, mode):
    """One glowtts_conv_wrw1_multi call -> [(problem, inputs, {name: tensor}, {name: start})]."""
    B, T = row.B, row.T
    names = LISTS[row.probs]
    D = Dev(mis="mask" if row.mis_mask else None)
    probs = (G.hip.Wrw1Problem * len(names))()
    mask_ptr = D.inp("mask", _inputs(names[0], kind, B, T).mask)
    meta = []
    for j, name in enumerate(names):
        p, I, q = _BY_NAME[name], _inputs(name, kind, B, T), probs[j]
        if row.odd_x_bs:                                                # two floats between the utterances: x_bs % 4 == 2
            xe = torch.cat([I.x.reshape(B, -1), I.gap[:, :2]], 1).reshape(-1)[: (B - 1) * (p.Cin * T + 2) + p.Cin * T]
            q.x, q.x_bs = D.inp(f"x{j}", xe), p.Cin * T + 2
        else:
            q.x, q.x_bs = D.inp(f"x{j}", I.xw), I.xw.shape[1] * T
        rows1 = I.d.shape[1]
        if p.d_strided:                                                 # eight floats between the utterances
            de = torch.cat([I.d.reshape(B, -1), I.gap], 1).reshape(-1)[: (B - 1) * (rows1 * T + 8) + rows1 * T]
            q.d, q.d_bs = D.inp(f"d{j}", de), rows1 * T + 8
        else:
            q.d, q.d_bs = D.inp(f"d{j}", I.d), rows1 * T
        q.d2, q.d2_bs = (D.inp(f"d2{j}", I.d2), (p.M - p.d_split) * T) if p.d_split else (None, 0)
        q.mask_d, q.mask_x = (mask_ptr if p.mask_d else None), (mask_ptr if p.mask_x else None)
        start = {"dwp": _start(p.Cin * p.M, j) if row.start else torch.zeros(p.Cin * p.M)}
        q.dwp = D.out(f"dwp{j}", (p.Cin, p.M), init=start["dwp"])
        if p.dbias:
            start["dbias"] = _start(p.M, 100 + j) if row.start else torch.zeros(p.M)
            q.dbias = D.out(f"dbias{j}", (p.M,), init=start["dbias"])
        q.Cin, q.M, q.d_split = p.Cin, p.M, p.d_split
        meta.append((p, I, j, start))
    assert G.lib.glowtts_conv_math(mode) == 0
    G.hip.set_knob("WRW1_CUS", row.cus)
    G.hip.set_knob("WRW1_XCD", row.xcd)
    G.hip.set_knob("WRW1_MULTI", row.multi)
    G.hip.call("glowtts_conv_wrw1_multi", len(names), ctypes.addressof(probs), B, T)
    r = D.finish()
    return [(p, I, {n: r[f"{n}{j}"] for n in start}, start) for p, I, j, start in meta]


@gpu
@pytest.mark.parametrize("row", ROW_PARAMS)
def test_wrw1_multi(G, row):
    """Counting inputs: every dwp and dbias EQUAL to fp64 in both modes; random inputs: within 1e-5 sum|term| per element."""
    assert set(_row_regimes(row)) == {row.regime}
    for kind in ("count", "random"):
        for mode in MODES:
            figs = []
            for p, I, got, start in _launch(G, row, kind, mode):
                want, cpu = _ref(p, I, F64), _ref(p, I, F32)
                for name, (value, terms) in want.items():
                    g, s = got[name].double(), start[name].double().reshape(value.shape)
                    what = f"wrw1 {row.name} {kind} mode {mode} {p.name} {name}"
                    assert bool(torch.isfinite(g).all()), what
                    if kind == "count":
                        assert float((terms + s.abs()).max()) < 2 ** 24, what
                        assert torch.equal(g, value + s), \
                            f"{what}: differs from integer arithmetic by up to {float((g - value - s).abs().max())} at " \
                            f"{[tuple(i.tolist()) for i in (g != value + s).nonzero()[:4]]}"
                        continue
                    sc = terms + s.abs()
                    err = (g - value - s).abs()
                    assert bool((err[sc == 0] == 0).all()), f"{what}: difference where every term is 0"
                    fig = float((err[sc > 0] / sc[sc > 0]).max())
                    share = float(((cpu[name][0].double() - value).abs()[terms > 0] / terms[terms > 0]).max())
                    figs.append(f"{p.name} {name} {fig:.1e} (fp32 CPU {share:.1e})")
                    assert fig <= RED_BOUND, f"{what}: {fig:.2e} of sum|term| > {RED_BOUND}"
            print(f"wrw1 {row.name} {kind} mode {mode} [{row.regime}]: " + ("all ==" if kind == "count" else
                                                                           "of sum|term|, bound 1e-5: " + "; ".join(figs)))


@gpu
def test_wrw1_multi_empty_batch_is_a_no_op(G):
    """B T = 0: nothing is launched and nothing is written, in both modes."""
    for mode in MODES:
        for B, T in ((0, 8), (2, 0)):
            D = Dev()
            probs = (G.hip.Wrw1Problem * 1)()
            q = probs[0]
            q.x, q.d = D.inp("x", torch.ones(64)), D.inp("d", torch.ones(64))
            q.dwp, q.dbias = D.out("dwp", (16,)), D.out("dbias", (4,))
            q.x_bs, q.d_bs, q.Cin, q.M = 16, 16, 4, 4
            assert G.lib.glowtts_conv_math(mode) == 0
            G.hip.call("glowtts_conv_wrw1_multi", 1, ctypes.addressof(probs), B, T)
            r = D.finish()
            assert bool((r["dwp"] == GUARD[F32]).all()) and bool((r["dbias"] == GUARD[F32]).all())


# =============================================================================================== CPU: regimes, bound
def test_rows_reach_their_split_regimes():
    """Every row takes the split regime it is there for, in every dispatch; all regimes and both dispatch counts are reached."""
    seen = set()
    for row in ROWS:
        regs = _row_regimes(row)
        assert set(regs) == {row.regime}, (row.name, regs)
        assert len(regs) == -(-len(LISTS[row.probs]) // MAX_BATCH)
        seen.add((row.regime, len(regs)))
    assert {r for r, _ in seen} == {"one", "steps", "empty", "fallback"}
    assert ("one", 2) in seen and ("steps", 2) in seen and ("steps", 1) in seen and ("empty", 1) in seen
    assert len(LISTS["eight"]) == 8 and len(LISTS["nine"]) == 9
    # the figures of the module docstring
    one = [_BY_NAME["16x16"]]
    assert _dispatch_mirror(one, 3, 164, 16, 1) == (16, 2, 18, 1) == _dispatch_mirror(one, 3, 164, 16, 0) == _dispatch_mirror(one, 3, 164, 20, 1)
    assert _dispatch_mirror(one, 3, 164, 20, 0) == (18, 1, 18, 1)
    assert _dispatch_mirror([_BY_NAME[n] for n in LISTS["eight"]], 2, 64, 80, 1)[3] == 15
    assert sum(-(-_BY_NAME[n].Cin // TK) * -(-_BY_NAME[n].M // TM) for n in LISTS["nine"][:8]) == 18
    # 15 tiles on a 256-CU chip, the only split count the older tests reach: 8 splits
    assert 256 // 2 // 15 == 8


def test_tables_cover_what_the_module_docstring_lists():
    shapes = {(p.Cin, p.M, p.d_split) for p in PROBLEMS}
    assert {(1, 1, 0), (16, 16, 0), (191, 127, 0), (192, 128, 0), (193, 129, 0), (192, 384, 192), (64, 320, 64), (200, 200, 0),
            (80, 192, 0)} <= shapes
    assert {(r.B, r.T) for r in ROWS} >= {(1, 4), (2, 32), (3, 36), (2, 64), (3, 164)}
    assert any(not p.dbias for p in PROBLEMS) and any(r.start for r in ROWS)
    assert all(r.B <= 17 and r.T <= 200 for r in ROWS) and all(p.Cin <= 384 and p.M <= 384 for p in PROBLEMS)
    assert int(_lengths(3, 36).min()) == 0 and int(_lengths(2, 32).min()) == 0
    for r in ROWS:                                       # the two-source form needs 16-byte rows in the one-by-one launches as well
        if r.T % 4 or r.odd_x_bs:
            assert not any(_BY_NAME[n].d_split for n in LISTS[r.probs])


def test_fp32_cpu_share_of_the_reduction_bound():
    """Plain fp32 torch on the CPU stays far inside 1e-5 sum|term| on the random inputs; counting inputs are exact in fp32."""
    worst = 0.0
    for B, T in ((1, 4), (2, 32), (3, 36), (2, 64), (3, 164)):
        for p in PROBLEMS:
            for kind in ("count", "random"):
                I = _inputs(p.name, kind, B, T)
                r64, r32 = _ref(p, I, F64), _ref(p, I, F32)
                for name, (value, terms) in r64.items():
                    if kind == "count":
                        assert float(terms.max()) < 2 ** 24 and torch.equal(r32[name][0].double(), value)
                    else:
                        ok = terms > 0
                        worst = max(worst, float(((r32[name][0].double() - value).abs()[ok] / terms[ok]).max()))
    print(f"fp32 CPU reductions: {worst:.1e} of sum|term| (bound {RED_BOUND})")
    assert worst <= RED_BOUND / 8
