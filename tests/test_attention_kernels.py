"""The encoder's relative-position attention one kernel output at a time, through the C ABI (glow_tts_train._hip.call:
glowtts_rel_attn_fwd_ex / _bwd_ex), against plain fp64 torch on the CPU, and the decision what to launch (csrc/attn_plan.hpp,
glowtts_attn_plan_for) on the CPU.  tests/test_hip_parity.py reaches these kernels through MultiHeadAttention against an fp32 torch
composition at rtol 1e-4 .. 5e-4 with 2 heads that share their embeddings: dq, dk, dv and ds are never seen there, only their sum
behind the projections, and a wrong key column in one 16-key tile or a head stride of 0 stays below those tolerances.  The GPU
tests are marked `gpu`; the tests at the end of the module are not.

Reference (index-based, none of the reference implementation's pad / reshape tricks), fp64:
    s[b,h,i,j] = (q_i.k_j + [|j-i| <= w] q_i.emb_k[h or 0][j-i+w]) / sqrt(dk); -1e4 where mask_i mask_j == 0 or |i-j| > block_len >= 0
    p = softmax_j s ; Pd = p * keep_byte * drop_scale ; out_i = sum_j Pd_ij v_j + sum_r Pd[i][i+r-w] emb_v[.][r]
    dP = (dout_i.v_j + [band] dout_i.emb_v[j-i+w]) * keep_byte * drop_scale ; ds = p (dP - sum_j p dP) / sqrt(dk) at kept pairs, 0 elsewhere
    dq_i = sum_j ds_ij k_j + sum_r ds[i][i+r-w] emb_k[r] ; dk_j = sum_i ds_ij q_i ; dv_j = sum_i Pd_ij dout_i
    demb_k[r] += sum_i ds[i][i+r-w] q_i ; demb_v[r] += sum_i Pd[i][i+r-w] dout_i   (over utterances, and heads when they share)
test_closed_form_backward_matches_autograd checks the backward formulas against fp64 autograd of the forward ones.

Each kernel on its own, so that an upstream error can neither cancel nor hide a downstream one: p_attn against fp64 from the
arguments; out against fp64 from THE KERNEL'S OWN p_attn (bit for bit what its phase 4 consumed); the backward takes p_attn as an
ARGUMENT (the fp64 softmax rounded once to fp32); ds from the arguments; dq, dk, demb_k from the kernel's own ds; dv, demb_v from
the arguments.  Rows marked e2e (one per form) are also checked from the arguments alone, native arithmetic, at the first-order
propagated bound (bound of the output + the upstream bound pushed through the contraction).  With bf16_mma = 1 the fp64 reference
rounds to bf16 (nearest even) exactly the operands include/glowtts_hip.h says the kernel rounds (forward: q, k, emb_k, Pd, v, emb_v;
backward: dout, v, emb_v, ds, k, emb_k, q and Pd as dK / dV use them); products of bf16 values are exact in fp32, so the bounds are
the native ones.  In the tiled form bf16_mma has no effect: the two calls must agree bit for bit (all but the atomically
accumulated demb_*).

Every launch (_Dev, as in tests/test_conv_kernels.py): each input is a copy in a guarded buffer and bit-identical afterwards, each
written output is pre-filled with GUARD between guards that survive, demb_k / demb_v start from 0, and from a running sum of small
integers at the rows marked start (one per form).  Lengths: row 0 full, from B >= 2 on one row of length 0, a third row partial;
q, k, v, dout hold random finite values beyond the length.  A fully masked query row gives p = 1/T on all T keys (what the
reference's -1e4 fill gives) and ds exactly 0; within a live row p and ds at masked or out-of-band pairs are exactly 0 (their
scale below is 0, and _units asserts equality there).

Two kinds of input.
  1. Selection inputs, asserted EQUAL: k_j = g * code(j) with a distinct +-1 code per key and a +-1 vector g per (utterance, head),
     q_i = 1024 g * code(pi(i)) for a chosen kept key pi(i), emb_k = 0.  The selected score leads every other by >= 2048 / sqrt(dk)
     >= 181 in scaled units, beyond where exp underflows to 0 in fp32 (the issue's 256 gives 45 at dk = 128: e^-45 = 2e-20 is not 0),
     so p_attn is exactly one-hot; all values are exact in bf16 and all sums in fp32.  v, emb_v, dout are integers in [-2, 2], keep
     bytes come with drop_scale = 2: out_i = keep * 2 * (v_pi(i) + [|pi(i)-i| <= w] emb_v[pi(i)-i+w]), dv and demb_v are integer sums,
     ds = dq = dk = demb_k = 0.  (dout is 0 on fully masked query rows: their uniform p = 1/T would add non-dyadic terms to the integer
     sums; those rows are left to kind 2.)  pi cycles through: the diagonal, +-w, +-(w+1), the first and last key, a key of the last
     partial 16-tile, a key of another 64-key tile, the band edges under block_len (test_selection_hits_every_target).
  2. Random inputs: q, k, v, dout ~ N(0, 1), emb ~ N dk^-1/2.  Bounds per element in units of u = 2^-24 times a scale:
         output   scale                                                                        fp32 CPU   bound   MI355X
         p_attn   p_ij (1 + |s_ij - max_i| + E_ij + sum_j' p_ij' E_ij')                          2.23 u     16 u    2.16 u
                  with E = sum_d |q||k| (+ |q||emb_k| on the band) / sqrt(dk), 0 at masked pairs
         out      sum_j |Pd||v| + sum_r |Pd[i][i+r-w]||emb_v|                                     7.16 u     32 u    7.14 u
         ds       p_ij (A_ij + |dP_ij| + |dot_i| + sum_j' p_ij' (A_ij' + |dP_ij'|)) / sqrt(dk)    2.06 u     16 u    2.25 u
                  with A = sum_d |dout||v| (+ |dout||emb_v| on the band), keep byte and drop_scale applied, dot_i = sum_j p dP
         dq       sum_j |ds||k| + sum_r |ds[i][i+r-w]||emb_k|                                     9.89 u     64 u   10.42 u
         dk       sum_i |ds||q|                                                                   9.39 u     64 u    9.90 u
         dv       sum_i |Pd||dout|                                                               10.92 u     64 u   10.92 u
     (fp32 CPU: the worse of two x86 hosts, which differ in the order of torch's sums: dq 6.84 / 9.89, dk 9.39 / 7.09, dv 10.92 / 6.67;
     MI355X: the worst figure of either arithmetic over the table in a run of this module; demb_k / demb_v there 4.1e-7 of sum|term|.
     The contractions sit near the CPU's figure because at T = 512 both sum hundreds of terms of alternating sign one after the other.)
     (the |s - max| term of p_attn: the kernels' __expf rounds its argument).  The bound is 4 x what plain fp32 torch on the CPU
     shows against fp64 on the same inputs (the reference alone, worst over the shape table), rounded up to a power of two: the
     kernels sum in another order.  test_bound_table_matches_fp32_cpu_evaluation recomputes the figures and asserts
     fig <= bound <= 16 fig, so a bound cannot be widened afterwards.  demb_k, demb_v (block sums + float atomics):
     |got - want| <= 1e-5 sum|term|, the project's figure for that pattern (tests/test_conv_kernels.py, tests/test_flow_kernels.py).
     Each GPU test prints its figures (-s).

Shapes: CASES below: each row is the smallest that takes a branch and says which; _mirror restates the rules of csrc/attn_plan.hpp
and labels every row, test_every_branch_is_reached asserts that the labels reached are exactly EXPECT, test_plans_agree_with_the_mirror
asks the library for every row, and test_plan_sweep sweeps the whole envelope the header promises.  B <= 3, H <= 3, T <= 577.
"""
import ctypes
import functools
import math
import types

import pytest
import torch

gpu = pytest.mark.gpu

U = 2.0 ** -24
GUARD = -1234.5
GUARD8 = 0xA5
PAD = 8
F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
LDS_MAX = 160 * 1024
AMP = 8192.0             # |q| of the selection inputs

# element-wise bounds in u (the table of the module docstring); reductions: RED of sum|term|
BOUNDS = {"p": 16, "out": 32, "ds": 16, "dq": 64, "dk": 64, "dv": 64}
RED = 1e-5
SHORT10, SHORT16, STRIP32, TILED = 1, 2, 3, 4
FORM = {SHORT10: "short10", SHORT16: "short16", STRIP32: "strip32", TILED: "tiled"}


# =============================================================================================== the shape table
def _case(name, why, B, H, T, dk, w, share=1, bl=-1, drop=None, **kw):
    """w = -1: no relative embeddings (NULL); drop: None, "exact" (bytes 0/1, drop_scale 2) or the dropout probability."""
    d = dict(e2e=False, start=False)
    d.update(kw)
    return types.SimpleNamespace(name=name, why=why, B=B, H=H, T=T, dk=dk, w=w, share=share, bl=bl, drop=drop, **d)


CASES = [
    _case("T1", "a single token", 1, 1, 1, 16, 0),
    _case("T5-w7", "window wider than the sentence; per-head embeddings", 1, 2, 5, 16, 7, share=0),
    _case("T15", "T < 16, T % 4 != 0: one partial tile, the scalar staging paths; an empty utterance", 2, 2, 15, 16, 2),
    _case("T16", "exactly one 16-key tile; exact keep bytes", 1, 1, 16, 48, 1, drop="exact"),
    _case("T17-bl3", "one key in the second tile; block band 3 narrower than window 4; 3 heads with their own embeddings", 2, 3, 17, 16,
          4, share=0, bl=3),
    _case("T63-dc24", "w = 4 / dk = 32: DC = 24, a partial second slab in the embedding gradients; dropout 0.1", 1, 1, 63, 32, 4,
          drop=0.1),
    _case("T64-none", "exactly one query block; no relative embeddings; block band 0 (the diagonal alone)", 1, 2, 64, 16, -1, bl=0),
    _case("T65-dk96", "second query block of one row; the dk = 96 instantiations", 2, 1, 65, 96, 4, e2e=True, start=True),
    _case("T160", "the production shape (NT = 10 at its limit): dk = 96, w = 4, dropout, length 70 of 160 crosses a query block", 3, 2,
          160, 96, 4, drop=0.1),
    _case("T161", "NT 10 -> 16; block band wider than T; T % 4 != 0", 1, 1, 161, 16, 2, bl=200, e2e=True, start=True),
    _case("T192-dk128", "dk = 128 at the last T whose probability strip fits LDS", 1, 1, 192, 128, 0),
    _case("T208-dk128", "dk = 128 / T = 208: the LDS strip does not fit (hole 1) -> strip in registers with 13 tiles; no embeddings", 1, 1,
          208, 128, -1),
    _case("T224-w0", "w = 0 / dk = 96 / T = 224: the embedding-gradient slab is capped (hole 2)", 1, 1, 224, 96, 0),
    _case("T240-dk112", "dk = 112 / T = 240: hole 1; exact keep bytes", 1, 1, 240, 112, 4, drop="exact", e2e=True, start=True),
    _case("T256-dk128", "dk = 128 / T = 256: hole 1 at the strip's last length; w = 7", 1, 1, 256, 128, 7),
    _case("T256-dk96-w1", "dk = 96 / T = 256 just fits the LDS strip; w = 1: hole 2 in the short form; per-head embeddings", 1, 2, 256,
          96, 1, share=0),
    _case("T257", "LDS strip -> register strip; T % 4 != 0 there", 1, 1, 257, 16, 2),
    _case("T320", "register strip, five 64-key tiles; exact keep bytes; block band 3; partial length", 3, 1, 320, 48, 4, drop="exact",
          bl=3),
    _case("T512-dk128", "the largest strip: dk = 128, w = 7 at T = 512", 1, 1, 512, 128, 7),
    _case("T512-dk96-w1", "hole 2: w = 1 / dk = 96 at T = 512", 1, 1, 512, 96, 1),
    _case("T512-dk48-w2", "hole 2: w = 2 / dk = 48 at T = 512; per-head embeddings", 1, 2, 512, 48, 2, share=0),
    _case("T513", "-> tiled kernels; per-head embeddings; dropout; T % 4 != 0", 1, 2, 513, 16, 4, share=0, drop=0.1, e2e=True,
          start=True),
    _case("T577", "tiled, ten 64-tiles with a partial last one; an empty utterance; block band 3", 2, 1, 577, 48, 2, bl=3),
]
BY_NAME = {c.name: c for c in CASES}

EXPECT = {"short10", "short16", "strip32", "tiled", "strip32:T<=256", "dk96", "dk-any", "rel", "no-rel", "shared", "per-head",
          "bl:none", "bl:0", "bl<w", "bl", "bl>=T", "drop:none", "drop:exact", "drop:p", "relgrad:one-slab", "relgrad:slabs", "relgrad:partial-slab",
          "relgrad:capped", "relgrad:per-offset", "w>=T", "T%4", "T%16", "T<16", "query-blocks>1", "key-tiles>1", "empty-utterance",
          "partial-length", "T=1", "w:0", "w:1", "w:2", "w:4", "w:7"}


def _lds_qblock(dk, T, regs):
    tp = -(-T // 16) * 16 + 4
    strip = 4 * 16 * 68 + 4 * 16 * 16 if regs else 64 * tp
    return 4 * (dk * 80 + dk * 68 + strip + 16 * (dk + 4) + 16 * (dk + 16) + 1088) + 64 * tp


def _lds_relgrad(nr, T, dc):
    return 4 * (2 * nr * T + 2 * dc * (T + 1))


def _mirror(T, dk, w, bf, bwd):
    """The rules of csrc/attn_plan.hpp (plan_attn) restated -> the fields of glowtts_attn_plan."""
    m = types.SimpleNamespace(form=0, dk96=int(dk == 96), bf16=0, lds_qblock=0, lds_dkv=0, lds_relgrad=0, relgrad_dc=0,
                              relgrad_grid_y=0, launches=0)
    rel = w >= 0
    if T > 512:
        m.form, m.launches = TILED, 3
        if bwd and rel:
            m.lds_relgrad, m.relgrad_grid_y, m.launches = 4 * T, 2 * w + 1, 5
    else:
        m.bf16, m.launches = int(bf), 1
        lds_strip = T <= 256 and _lds_qblock(dk, T, False) <= LDS_MAX
        m.form = STRIP32 if not lds_strip else SHORT10 if T <= 160 else SHORT16
        m.lds_qblock = _lds_qblock(dk, T, not lds_strip)
        if bwd and rel:
            nr = 2 * w + 1
            dc = min(dk, (256 // nr) & ~7)
            while dc > 8 and _lds_relgrad(nr, T, dc) > LDS_MAX:
                dc -= 8
            m.relgrad_dc, m.relgrad_grid_y, m.lds_relgrad = dc, -(-dk // dc), _lds_relgrad(nr, T, dc)
            m.launches += 1
    if bwd:
        m.lds_dkv = 4 * (2 * dk * 68 + 2 * 64 * 80)
        m.launches += 1
    return m


@functools.lru_cache(maxsize=None)
def _labels(name):
    c = BY_NAME[name]
    m = _mirror(c.T, c.dk, c.w, False, True)
    L = {FORM[m.form], "dk96" if m.dk96 else "dk-any", "rel" if c.w >= 0 else "no-rel"}
    if m.form == STRIP32 and c.T <= 256:
        L.add("strip32:T<=256")
    if c.w >= 0:
        L.add("shared" if c.share else "per-head")
        L.add(f"w:{c.w}")
        if c.w >= c.T:
            L.add("w>=T")
        if m.form == TILED:
            L.add("relgrad:per-offset")
        else:
            uncapped = min(c.dk, (256 // (2 * c.w + 1)) & ~7)
            L.add("relgrad:capped" if m.relgrad_dc < uncapped else "relgrad:partial-slab" if c.dk % m.relgrad_dc else "relgrad:one-slab"
                  if m.relgrad_grid_y == 1 else "relgrad:slabs")
    L.add("bl:none" if c.bl < 0 else "bl:0" if c.bl == 0 else "bl>=T" if c.bl >= c.T else "bl<w" if c.bl < c.w else "bl")
    L.add("drop:none" if c.drop is None else "drop:exact" if c.drop == "exact" else "drop:p")
    if c.T % 4:
        L.add("T%4")
    if c.T % 16:
        L.add("T%16")
    if c.T < 16:
        L.add("T<16")
    if c.T == 1:
        L.add("T=1")
    if c.T > 64:
        L.update({"query-blocks>1", "key-tiles>1"})
    if c.B >= 2:
        L.add("empty-utterance")
    if c.B >= 3:
        L.add("partial-length")
    return frozenset(L)


# =============================================================================================== small helpers
def _gen(name, salt=0):
    return torch.Generator().manual_seed((sum((i + 1) * 7919 * ord(ch) for i, ch in enumerate(name)) + 104729 * salt) % (2 ** 31))


def _lengths(c):
    """Row 0 full; from two rows on one row of length 0; a third row ends inside a 16-key tile (70 of 160: past a query block)."""
    L = torch.full((c.B,), c.T, dtype=torch.long)
    if c.B >= 2:
        L[c.B // 2] = 0
    if c.B >= 3:
        L[2] = (c.T * 7) // 16
        assert L[2] % 16 != 0
    return L


def _units(got, want, scale):
    """max over elements of |got - want| / (u * scale); where the scale is 0 the values must agree exactly."""
    got, want, scale = got.detach().double().reshape(-1), want.detach().double().reshape(-1), scale.detach().double().reshape(-1)
    err = (got - want).abs()
    zero = scale == 0
    assert bool((err[zero] == 0).all()), "difference where the scale is zero (masked / out-of-band pairs must be exact)"
    if bool(zero.all()):
        return 0.0
    return float((err[~zero] / (U * scale[~zero])).max())


def _red_fig(got, want, terms):
    err, sc = (got.detach().double() - want.double()).abs().reshape(-1), terms.double().reshape(-1)
    assert bool((err[sc == 0] == 0).all()), "difference where every term is 0"
    return float((err[sc > 0] / sc[sc > 0]).max()) if bool((sc > 0).any()) else 0.0


def _bits_equal(a, b):
    if a.dtype == torch.uint8:
        return a.shape == b.shape and torch.equal(a, b)
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _rb(x, bf):
    """bf16 rounding (nearest even) of fp32-representable values, kept in x's type."""
    return x.to(BF16).to(x.dtype) if bf else x


# =============================================================================================== inputs
def _code(T, dk):
    """A distinct +-1 code of length dk per key: the ten low bits of j, then bits of a hash of j."""
    j = torch.arange(T)
    bits = [(j >> b) & 1 for b in range(10)] + [((j * 2654435761 + 12345) >> (3 + b)) & 1 for b in range(dk - 10)]
    code = torch.stack(bits, 0).float() * 2 - 1                      # (dk, T)
    assert len({tuple(col.tolist()) for col in code[:10].t()}) == T
    return code


def _pi_targets(c, i, h, n):
    """Candidate keys of query i (may be invalid: filtered by the caller), rotated by the head so that heads differ."""
    w = max(c.w, 0)
    cand = [i, i + w, i - w, i + w + 1, i - w - 1, 0, n - 1, n - 1 - (n - 1) % 16, i + 64, i - 64]
    if c.bl >= 0:
        cand += [i + c.bl, i - c.bl]
    return cand[(i + h) % len(cand)]


@functools.lru_cache(maxsize=None)
def _pi(name):
    """pi[b][h][i]: the kept key query i selects (the diagonal where the candidate is not a kept key); -1 on masked rows."""
    c = BY_NAME[name]
    L = _lengths(c)
    pi = torch.full((c.B, c.H, c.T), -1, dtype=torch.long)
    for b in range(c.B):
        n = int(L[b])
        for h in range(c.H):
            for i in range(n):
                j = _pi_targets(c, i, h, n)
                ok = 0 <= j < n and (c.bl < 0 or abs(j - i) <= c.bl)
                pi[b, h, i] = j if ok else i
    return pi


@functools.lru_cache(maxsize=None)
def _inputs(name, kind):
    c = BY_NAME[name]
    g = _gen(name, 1 if kind == "random" else 2)
    B, H, T, dk, C = c.B, c.H, c.T, c.dk, c.H * c.dk
    nr, n_rel = 2 * c.w + 1, (1 if c.share else c.H)
    L = _lengths(c)
    I = types.SimpleNamespace(kind=kind, lengths=L, mask=(torch.arange(T)[None] < L[:, None]).float(), emb_k=None, emb_v=None,
                              drop=None, drop_scale=1.0)
    live = I.mask.bool()[:, None, None, :]                                              # (B, 1, 1, T)
    if kind == "random":
        I.q, I.k, I.v, I.dout = (torch.randn(B, C, T, generator=g) for _ in range(4))
        if c.w >= 0:
            I.emb_k = torch.randn(n_rel, nr, dk, generator=g) * dk ** -0.5
            I.emb_v = torch.randn(n_rel, nr, dk, generator=g) * dk ** -0.5
    else:
        code = _code(T, dk)                                                             # (dk, T)
        sign = (torch.randint(0, 2, (B, H, dk, 1), generator=g) * 2 - 1).float()
        pi = _pi(name)
        k = sign * code[None, None]
        q = AMP * sign * code[:, pi.clamp_min(0)].permute(1, 2, 0, 3)                   # (dk, B, H, T) -> (B, H, dk, T)
        rnd = torch.randn(2, B, H, dk, T, generator=g)
        I.q = torch.where(live, q, rnd[0]).reshape(B, C, T)
        I.k = torch.where(live, k, rnd[1]).reshape(B, C, T)
        I.v = torch.randint(-2, 3, (B, C, T), generator=g).float()
        I.dout = torch.randint(-2, 3, (B, C, T), generator=g).float() * I.mask[:, None, :]
        if c.w >= 0:
            I.emb_k = torch.zeros(n_rel, nr, dk)
            I.emb_v = torch.randint(-2, 3, (n_rel, nr, dk), generator=g).float()
    if c.drop is not None:
        pkeep = 0.5 if (c.drop == "exact" or kind == "select") else 1.0 - c.drop
        I.drop = (torch.rand(B, H, T, T, generator=g) < pkeep).to(torch.uint8)
        I.drop[:, :, min(3, T - 1), :] = 0                                              # a query row whose keep bytes are all 0
        I.drop_scale = 2.0 if pkeep == 0.5 else float(torch.tensor(1.0 / pkeep, dtype=F32))
    return I


# =============================================================================================== the reference
class _Ref:
    """The formulas of the module docstring for one case in dtype dt; bf: round the operands the bf16 kernels round."""

    def __init__(self, c, I, dt, bf=False):
        self.c, self.I, self.dt, self.bf = c, I, dt, bf
        B, H, T, dk = c.B, c.H, c.T, c.dk
        self.h = lambda x: x.to(dt).reshape(B, H, dk, T)
        self.rs = 1.0 / math.sqrt(dk)
        i, j = torch.arange(T)[:, None], torch.arange(T)[None]
        m = I.mask.bool()
        self.keep = (m[:, None, :, None] & m[:, None, None, :]) & ((j - i).abs() <= c.bl if c.bl >= 0 else torch.ones(T, T, dtype=torch.bool))
        self.keep = self.keep.expand(B, H, T, T)
        self.rel = c.w >= 0
        if self.rel:
            nr = 2 * c.w + 1
            ridx = j - i + c.w
            self.inband = (ridx >= 0) & (ridx <= 2 * c.w)
            self.ridx = ridx.clamp(0, 2 * c.w).expand(B, H, T, T)
            jidx = i + torch.arange(nr)[None] - c.w
            self.jvalid = (jidx >= 0) & (jidx < T)
            self.jidx = jidx.clamp(0, T - 1).expand(B, H, T, nr)
            self.ek = I.emb_k.to(dt).expand(H, nr, dk)
            self.ev = I.emb_v.to(dt).expand(H, nr, dk)
        self.kb = None if I.drop is None else I.drop != 0

    def band(self, R):          # (B, H, T, nr) -> (B, H, T, T): R[i][j-i+w] on the band, 0 elsewhere
        return torch.where(self.inband, R.gather(-1, self.ridx), torch.zeros((), dtype=R.dtype))

    def diag(self, M):          # (B, H, T, T) -> (B, H, T, nr): M[i][i+r-w], 0 outside the sentence
        return M.gather(-1, self.jidx) * self.jvalid

    def dropped(self, p32):
        """Pd as every kernel forms it: ONE fp32 product p * drop_scale at kept bytes (p32: fp32 tensor) -> dt."""
        if self.kb is None:
            return p32.to(self.dt)
        return torch.where(self.kb, p32.float() * torch.tensor(self.I.drop_scale, dtype=F32), torch.zeros((), dtype=F32)).to(self.dt)

    def drop64(self, x):
        """x * keep_byte * drop_scale in dt (no fp32 product)."""
        return x if self.kb is None else torch.where(self.kb, x * self.I.drop_scale, torch.zeros((), dtype=self.dt))

    def contract(self, a, b, e, rnd=True):
        """sum_d a[d][i] b[d][j] + band(sum_d a[d][i] e[r][d]) and the same of absolute values."""
        bf = self.bf and rnd
        a, b = _rb(self.h(a), bf), _rb(self.h(b), bf)
        s, S = torch.einsum("bhdi,bhdj->bhij", a, b), torch.einsum("bhdi,bhdj->bhij", a.abs(), b.abs())
        if self.rel:
            e = _rb(e, bf)
            s = s + self.band(torch.einsum("bhdi,hrd->bhir", a, e))
            S = S + self.band(torch.einsum("bhdi,hrd->bhir", a.abs(), e.abs()))
        return s, S

    def apply(self, M, b, e):
        """out[d][i] = sum_j M[i][j] b[d][j] + sum_r M[i][i+r-w] e[r][d] -> (B, C, T), and the same of absolute values."""
        M, b = _rb(M, self.bf), _rb(self.h(b), self.bf)
        o, O = torch.einsum("bhij,bhdj->bhdi", M, b), torch.einsum("bhij,bhdj->bhdi", M.abs(), b.abs())
        if self.rel:
            e, W = _rb(e, self.bf), self.diag(M)
            o = o + torch.einsum("bhir,hrd->bhdi", W, e)
            O = O + torch.einsum("bhir,hrd->bhdi", W.abs(), e.abs())
        shape = (self.c.B, self.c.H * self.c.dk, self.c.T)
        return o.reshape(shape), O.reshape(shape)

    def applyT(self, M, a):
        """out[d][j] = sum_i M[i][j] a[d][i] -> (B, C, T), and the same of absolute values."""
        M, a = _rb(M, self.bf), _rb(self.h(a), self.bf)
        shape = (self.c.B, self.c.H * self.c.dk, self.c.T)
        return (torch.einsum("bhij,bhdi->bhdj", M, a).reshape(shape), torch.einsum("bhij,bhdi->bhdj", M.abs(), a.abs()).reshape(shape))

    def emb_grad(self, M, a):
        """dE[h or 0][r][d] = sum_b (sum_h) sum_i M[i][i+r-w] a[d][i] (nothing rounded) and the sum of |terms|."""
        W, a = self.diag(M), self.h(a)
        t, Tm = torch.einsum("bhir,bhdi->hrd", W, a), torch.einsum("bhir,bhdi->hrd", W.abs(), a.abs())
        return (t.sum(0, keepdim=True), Tm.sum(0, keepdim=True)) if self.c.share else (t, Tm)

    # ---- forward
    def scores(self):
        s, S = self.contract(self.I.q, self.I.k, self.ek if self.rel else None)
        fill = torch.full((), -1e4, dtype=self.dt)
        return torch.where(self.keep, s * self.rs, fill), torch.where(self.keep, S * self.rs, torch.zeros((), dtype=self.dt))

    def p(self):
        """p_attn and its scale."""
        s, E = self.scores()
        p = torch.softmax(s, -1)
        mx = s.max(-1, keepdim=True).values
        return p, p * (1 + (s - mx).abs() + E + (p * E).sum(-1, keepdim=True))

    def out(self, p32):
        return self.apply(self.dropped(p32), self.I.v, self.ev if self.rel else None)

    # ---- backward
    def ds(self, p32):
        """ds, its scale, and dP after dropout (p32: the p_attn argument, fp32)."""
        p = p32.to(self.dt)
        dP, A = self.contract(self.I.dout, self.I.v, self.ev if self.rel else None)
        if self.kb is not None:
            sc = torch.tensor(self.I.drop_scale, dtype=self.dt)
            zero = torch.zeros((), dtype=self.dt)
            dP, A = torch.where(self.kb, dP * sc, zero), torch.where(self.kb, A * sc, zero)
        dot = (p * dP).sum(-1, keepdim=True)
        zero = torch.zeros((), dtype=self.dt)
        ds = torch.where(self.keep, p * (dP - dot) * self.rs, zero)
        scale = torch.where(self.keep, p * (A + dP.abs() + dot.abs() + (p * (A + dP.abs())).sum(-1, keepdim=True)) * self.rs, zero)
        return ds, scale

    def dq(self, ds):
        return self.apply(ds.to(self.dt), self.I.k, self.ek if self.rel else None)

    def dk(self, ds):
        return self.applyT(ds.to(self.dt), self.I.q)

    def dv(self, p32):
        return self.applyT(self.dropped(p32), self.I.dout)

    def demb_k(self, ds):
        return self.emb_grad(ds.to(self.dt), self.I.q)

    def demb_v(self, p32):
        return self.emb_grad(self.dropped(p32), self.I.dout)


@functools.lru_cache(maxsize=None)
def _p_arg(name, kind):
    """The p_attn ARGUMENT of the backward: the fp64 softmax rounded once to fp32 (native scores)."""
    c = BY_NAME[name]
    return _Ref(c, _inputs(name, kind), F64).p()[0].float()


# =============================================================================================== the launches
class _Dev:
    """The buffers of one raw-ABI call: inputs are copies inside guarded buffers (bit-identical afterwards), outputs live between
    GUARD sentinels."""

    def __init__(self):
        self.ins, self.outs = [], {}

    @staticmethod
    def _place(numel, dtype):
        pad = PAD if dtype == torch.float32 else 4 * PAD
        buf = torch.full((numel + 2 * pad,), GUARD if dtype == torch.float32 else GUARD8, device="cuda", dtype=dtype)
        assert buf.data_ptr() % 16 == 0
        return buf, buf[pad: pad + numel], pad

    def inp(self, name, t):
        if t is None:
            return None
        t = t.contiguous()
        buf, view, lo = self._place(t.numel(), t.dtype)
        view.copy_(t.reshape(-1))
        self.ins.append((name, t, buf, lo))
        return view.data_ptr()

    def out(self, name, shape, init=None):
        numel = int(math.prod(shape))
        buf, view, lo = self._place(numel, torch.float32)
        if init is not None:
            view.copy_(init.reshape(-1).float())
        self.outs[name] = (buf, lo, numel, tuple(shape))
        return view.data_ptr()

    def finish(self):
        torch.cuda.synchronize()
        for name, t, buf, lo in self.ins:
            b = buf.cpu()
            g = GUARD if t.dtype == torch.float32 else GUARD8
            assert _bits_equal(b[lo: lo + t.numel()], t.reshape(-1)), f"input {name} changed"
            assert bool((b[:lo] == g).all()) and bool((b[lo + t.numel():] == g).all()), f"written around input {name}"
        res = {}
        for name, (buf, lo, numel, shape) in self.outs.items():
            b = buf.cpu()
            assert bool((b[:lo] == GUARD).all()) and bool((b[lo + numel:] == GUARD).all()), f"guard of output {name} overwritten"
            res[name] = b[lo: lo + numel].clone().reshape(shape)
            assert bool(torch.isfinite(res[name]).all()), f"non-finite output {name}"
        return types.SimpleNamespace(**res)

    def untouched(self, what):
        torch.cuda.synchronize()
        for name, (buf, lo, numel, shape) in self.outs.items():
            assert bool((buf.cpu() == GUARD).all()), f"{what}: output {name} touched"


@pytest.fixture()
def G():
    from glow_tts_train import _hip

    return types.SimpleNamespace(hip=_hip, lib=_hip.load())


def _start(shape, salt):
    return torch.randint(1, 4, shape, generator=_gen("start", salt)).float()


def _emb_shape(c):
    return (1 if c.share else c.H, 2 * c.w + 1, c.dk)


def _run_fwd(G, c, I, bf):
    D = _Dev()
    args = [D.inp(n, getattr(I, n)) for n in ("q", "k", "v", "emb_k", "emb_v", "mask", "drop")]
    args += [I.drop_scale, D.out("p", (c.B, c.H, c.T, c.T)), D.out("out", (c.B, c.H * c.dk, c.T)),
             c.B, c.H, c.T, c.dk, c.w if c.w >= 0 else 2, c.share, c.bl, bf]
    G.hip.call("glowtts_rel_attn_fwd_ex", *args)
    return D.finish()


def _run_bwd(G, c, I, p_arg, bf, start=None):
    D = _Dev()
    args = [D.inp(n, getattr(I, n)) for n in ("dout", "q", "k", "v", "emb_k", "emb_v", "mask", "drop")]
    args += [I.drop_scale, D.inp("p_attn", p_arg)]
    args += [D.out("ds", (c.B, c.H, c.T, c.T))] + [D.out(n, (c.B, c.H * c.dk, c.T)) for n in ("dq", "dk", "dv")]
    if c.w >= 0:
        z = torch.zeros(_emb_shape(c))
        args += [D.out("demb_k", _emb_shape(c), init=z if start is None else start[0]),
                 D.out("demb_v", _emb_shape(c), init=z if start is None else start[1])]
    else:
        args += [None, None]
    args += [c.B, c.H, c.T, c.dk, c.w if c.w >= 0 else 2, c.share, c.bl, bf]
    G.hip.call("glowtts_rel_attn_bwd_ex", *args)
    return D.finish()


def _elem(figs, what, key, got, want, scale, extra=None):
    """Assert got within BOUNDS[key] u of want (extra: an absolute per-element allowance on top, the propagated upstream bound)."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if extra is None:
        fig = _units(got, want, scale)
        figs.append(f"{what} {fig:.2f} u (bound {BOUNDS[key]})")
        assert fig <= BOUNDS[key], f"{what}: {fig:.2f} u > {BOUNDS[key]} u"
    else:
        err, allow = (got.double() - want).abs(), BOUNDS[key] * U * scale + extra
        fig = float((err / allow.clamp_min(1e-300)).max())
        figs.append(f"{what} {fig:.2f} of the propagated bound")
        assert bool((err <= allow).all()), f"{what}: {fig:.2f} x the propagated bound"


def _red(figs, what, got, want, terms, start=None, extra=None):
    got = got.double() - (0 if start is None else start.double())
    if extra is None:
        fig = _red_fig(got, want, terms)
        figs.append(f"{what} {fig:.1e} of sum|term| (bound {RED:.0e})")
        assert fig <= RED, f"{what}: {fig:.2e} of sum|term| > {RED:.0e}"
    else:
        err, allow = (got - want).abs(), RED * terms + extra
        figs.append(f"{what} {float((err / allow.clamp_min(1e-300)).max()):.2f} of the propagated bound")
        assert bool((err <= allow).all()), what


# =============================================================================================== the GPU tests
@gpu
@pytest.mark.parametrize("bf", (0, 1), ids=("fp32", "bf16"))
@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_forward_random(G, name, bf):
    c, I = BY_NAME[name], _inputs(name, "random")
    tiled = "tiled" in _labels(name)
    got = _run_fwd(G, c, I, bf)
    figs = []
    R = _Ref(c, I, F64, bf=bool(bf) and not tiled)
    p, p_scale = R.p()
    _elem(figs, "p_attn", "p", got.p, p, p_scale)
    dead = ~I.mask.bool()
    if bool(dead.any()):                                  # fully masked query rows: the reference's uniform 1/T, to the bound above
        rows = got.p.double()[dead[:, None, :].expand(c.B, c.H, c.T)]
        assert float((rows - 1.0 / c.T).abs().max()) <= BOUNDS["p"] * U / c.T
    out, out_scale = R.out(got.p)                         # from the kernel's OWN p_attn
    _elem(figs, "out", "out", got.out, out, out_scale)
    if c.e2e and not bf:                                  # from the arguments alone: + the bound of p pushed through the contraction
        Pd = R.drop64(p)
        want, sc = R.apply(Pd, I.v, R.ev if R.rel else None)
        dPd = R.drop64(BOUNDS["p"] * U * p_scale) + U * Pd            # the bound of p, and the rounding of the product p * drop_scale
        _, extra = R.apply(dPd, I.v, R.ev if R.rel else None)
        _elem(figs, "out(e2e)", "out", got.out, want, sc, extra=extra)
    if tiled and bf:
        ref = _run_fwd(G, c, I, 0)
        assert _bits_equal(got.p, ref.p) and _bits_equal(got.out, ref.out), "bf16_mma changed the tiled form"
        figs.append("bf16_mma == fp32 bit for bit")
    print(f"\n  {name} [{'bf16' if bf else 'fp32'}] {sorted(_labels(name))}\n    " + "; ".join(figs))


@gpu
@pytest.mark.parametrize("bf", (0, 1), ids=("fp32", "bf16"))
@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_backward_random(G, name, bf):
    c, I = BY_NAME[name], _inputs(name, "random")
    tiled = "tiled" in _labels(name)
    p_arg = _p_arg(name, "random")
    start = (_start(_emb_shape(c), 1), _start(_emb_shape(c), 2)) if (c.start and c.w >= 0) else None
    got = _run_bwd(G, c, I, p_arg, bf, start)
    figs = []
    R = _Ref(c, I, F64, bf=bool(bf) and not tiled)
    ds, ds_scale = R.ds(p_arg)
    _elem(figs, "ds", "ds", got.ds, ds, ds_scale)
    assert bool((got.ds[~R.keep] == 0).all()), "ds not exactly 0 at a masked or out-of-band pair"
    for key, fn in (("dq", R.dq), ("dk", R.dk)):          # from the kernel's OWN ds
        want, sc = fn(got.ds)
        _elem(figs, key, key, getattr(got, key), want, sc)
    want, sc = R.dv(p_arg)
    _elem(figs, "dv", "dv", got.dv, want, sc)
    if c.w >= 0:
        want, terms = R.demb_k(got.ds)
        _red(figs, "demb_k", got.demb_k, want, terms, None if start is None else start[0])
        want, terms = R.demb_v(p_arg)
        _red(figs, "demb_v", got.demb_v, want, terms, None if start is None else start[1])
    if c.e2e and not bf:                                  # dq, dk, demb_k from the arguments: + the bound of ds pushed through
        dds = BOUNDS["ds"] * U * ds_scale
        for key, fn in (("dq", R.dq), ("dk", R.dk)):
            (want, sc), (_, extra) = fn(ds), fn(dds)
            _elem(figs, f"{key}(e2e)", key, getattr(got, key), want, sc, extra=extra)
        if c.w >= 0:
            (want, terms), (_, extra) = R.demb_k(ds), R.demb_k(dds)
            _red(figs, "demb_k(e2e)", got.demb_k, want, terms, None if start is None else start[0], extra=extra)
    if tiled and bf:
        ref = _run_bwd(G, c, I, p_arg, 0, start)
        for key in ("ds", "dq", "dk", "dv"):
            assert _bits_equal(getattr(got, key), getattr(ref, key)), f"bf16_mma changed {key} of the tiled form"
        figs.append("bf16_mma == fp32 bit for bit")
    print(f"\n  {name} [{'bf16' if bf else 'fp32'}] {sorted(_labels(name))}\n    " + "; ".join(figs))


def _select_expect(c, I):
    """What the selection inputs must give exactly, from the index arithmetic alone (no softmax, no contraction):
    p one-hot at pi on live rows; out, dv, demb_v."""
    B, H, T, dk = c.B, c.H, c.T, c.dk
    pi = _pi(c.name)
    live = pi >= 0                                                                          # (B, H, T)
    p = torch.zeros(B, H, T, T, dtype=F64)
    p.scatter_(-1, pi.clamp_min(0)[..., None], live[..., None].double())
    ks = torch.ones(B, H, T, dtype=F64) if I.drop is None else \
        I.drop.gather(-1, pi.clamp_min(0)[..., None])[..., 0].double() * I.drop_scale       # keep * scale at (i, pi(i))
    ks = ks * live
    v, dout = I.v.double().reshape(B, H, dk, T), I.dout.double().reshape(B, H, dk, T)
    vsel = v.gather(-1, pi.clamp_min(0)[:, :, None, :].expand(B, H, dk, T))                 # v[:, pi(i)]
    out = ks[:, :, None, :] * vsel
    dv = torch.zeros(B, H, dk, T, dtype=F64)
    dv.scatter_add_(-1, pi.clamp_min(0)[:, :, None, :].expand(B, H, dk, T), ks[:, :, None, :] * dout)
    demb_v = None
    if c.w >= 0:
        nr = 2 * c.w + 1
        r = pi - torch.arange(T) + c.w                                                      # (B, H, T)
        inb = live & (r >= 0) & (r < nr)
        ev = I.emb_v.double().expand(H, nr, dk)
        esel = ev[torch.arange(H)[None, :, None], r.clamp(0, nr - 1)]                       # (B, H, T, dk)
        out = out + (ks * inb)[:, :, None, :] * esel.permute(0, 1, 3, 2)
        demb_v = torch.zeros(H, nr, dk, dtype=F64)
        onehot = torch.zeros(B, H, T, nr, dtype=F64).scatter_(-1, r.clamp(0, nr - 1)[..., None], (ks * inb)[..., None])
        demb_v = torch.einsum("bhir,bhdi->hrd", onehot, dout)
        if c.share:
            demb_v = demb_v.sum(0, keepdim=True)
    return types.SimpleNamespace(p=p, live=live, out=out.reshape(B, H * dk, T), dv=dv.reshape(B, H * dk, T), demb_v=demb_v)


def _exact(what, got, want):
    assert torch.equal(got.double(), want.double()), \
        f"{what}: differs from the index arithmetic by up to {float((got.double() - want).abs().max())} at " \
        f"{[tuple(i.tolist()) for i in (got.double() != want.double()).nonzero()[:4]]}"


@gpu
@pytest.mark.parametrize("bf", (0, 1), ids=("fp32", "bf16"))
@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_selection_is_exact(G, name, bf):
    """Kind 1: p_attn one-hot at the chosen key, out / dv / demb_v the integer sums, ds = dq = dk = demb_k = 0: all EQUAL."""
    c, I = BY_NAME[name], _inputs(name, "select")
    E = _select_expect(c, I)
    f = _run_fwd(G, c, I, bf)
    lv = E.live[..., None].expand_as(E.p)
    _exact("p_attn on live rows", torch.where(lv, f.p.double(), E.p), E.p)
    assert float((f.p.double()[~lv] - 1.0 / c.T).abs().max() if bool((~lv).any()) else 0.0) <= BOUNDS["p"] * U / c.T
    lo = E.live[:, :, None, :].expand(c.B, c.H, c.dk, c.T).reshape(E.out.shape)
    _exact("out on live rows", torch.where(lo, f.out.double(), E.out), E.out)
    p_arg = torch.where(lv, E.p, torch.full((), 1.0 / c.T, dtype=F64)).float()
    b = _run_bwd(G, c, I, p_arg, bf)
    for key in ("ds", "dq", "dk"):
        _exact(key, getattr(b, key), torch.zeros_like(getattr(b, key)))
    _exact("dv", b.dv, E.dv)
    if c.w >= 0:
        _exact("demb_k", b.demb_k, torch.zeros_like(b.demb_k))
        _exact("demb_v", b.demb_v, E.demb_v)


@gpu
@pytest.mark.parametrize("B,T", [(0, 8), (2, 0)], ids=["B0", "T0"])
def test_empty_batch_or_no_tokens_is_a_no_op(G, B, T):
    for bf in (0, 1):
        D = _Dev()
        x = [D.out(n, (2, 32, 8)) for n in ("q", "k", "v", "dout", "out", "dq", "dk", "dv")]
        e = [D.out(n, (1, 5, 16)) for n in ("emb_k", "emb_v", "demb_k", "demb_v")]
        m, p, ds = D.out("mask", (2, 8)), D.out("p", (2, 2, 8, 8)), D.out("ds", (2, 2, 8, 8))
        G.hip.call("glowtts_rel_attn_fwd_ex", x[0], x[1], x[2], e[0], e[1], m, None, 1.0, p, x[4], B, 2, T, 16, 2, 1, -1, bf)
        G.hip.call("glowtts_rel_attn_bwd_ex", x[3], x[0], x[1], x[2], e[0], e[1], m, None, 1.0, p, ds, x[5], x[6], x[7], e[2], e[3],
                   B, 2, T, 16, 2, 1, -1, bf)
        D.untouched(f"B={B} T={T}")


@gpu
def test_abi_rejects_before_any_launch(G):
    """dk = 24, dk = 144, window = 8, emb_k without demb_k: an error code, glowtts_last_error set, nothing written."""
    for what, dk, w, demb, match in (("dk=24", 24, 2, True, "multiple of 16"), ("dk=144", 144, 2, True, "multiple of 16"),
                                     ("window=8", 16, 8, True, "window 8"), ("demb_k NULL", 16, 2, False, "need their gradients")):
        D = _Dev()
        x = [D.out(n, (2, 2 * 144, 8)) for n in ("q", "k", "v", "dout", "out", "dq", "dk", "dv")]
        e = [D.out(n, (1, 17, 144)) for n in ("emb_k", "emb_v", "demb_k", "demb_v")]
        m, p, ds = D.out("mask", (2, 8)), D.out("p", (2, 2, 8, 8)), D.out("ds", (2, 2, 8, 8))
        calls = [("glowtts_rel_attn_bwd_ex", (x[3], x[0], x[1], x[2], e[0], e[1], m, None, 1.0, p, ds, x[5], x[6], x[7],
                                              e[2] if demb else None, e[3], 2, 2, 8, dk, w, 1, -1, 0))]
        if demb:
            calls.append(("glowtts_rel_attn_fwd_ex", (x[0], x[1], x[2], e[0], e[1], m, None, 1.0, p, x[4], 2, 2, 8, dk, w, 1, -1, 0)))
        for fn, args in calls:
            with pytest.raises(RuntimeError, match=match):
                G.hip.call(fn, *args)
            assert match in G.lib.glowtts_last_error().decode()
        D.untouched(what)


# =============================================================================================== the tables, on the CPU
def _plan(lib, hip, T, dk, w, bf, bwd):
    out = hip.AttnPlan()
    rc = lib.glowtts_attn_plan_for(T, dk, w, bf, bwd, ctypes.byref(out))
    assert rc == 0, lib.glowtts_last_error().decode()
    return out


_FIELDS = ("form", "dk96", "bf16", "lds_qblock", "lds_dkv", "lds_relgrad", "relgrad_dc", "relgrad_grid_y", "launches")


def test_plan_sweep():
    """dk in {16 .. 128} x window in {-1, 0 .. 7} x T in 1 .. 1100 x forward / backward x both arithmetics through
    glowtts_attn_plan_for (no device is touched): every LDS figure <= 160 KiB, the tiled form exactly for T > 512, and where the
    slab reduction of the embedding gradients runs (backward with a window, T <= 512) DC is a positive multiple of 8 or dk and
    (2w+1) DC <= 256.  With the rules as they were before csrc/attn_plan.hpp this sweep fails (the next test computes them): the
    q-block kernel's 169 472 B at dk = 112 and 180 992 B at dk = 128 for T = 256 (over the limit from T = 225 / 193), the
    embedding-gradient slab's 217 472 B at window 2, dk >= 48, T = 512 (from T = 386), window 1 / dk >= 80 from T = 246, window 0 /
    dk = 96 from T = 211."""
    from glow_tts_train import _hip

    lib = _hip.load()
    out = _hip.AttnPlan()
    ref, fn = ctypes.byref(out), lib.glowtts_attn_plan_for
    for dk in range(16, 129, 16):
        for w in range(-1, 8):
            for bwd in (0, 1):
                for bf in (0, 1):
                    for T in range(1, 1101):
                        assert fn(T, dk, w, bf, bwd, ref) == 0
                        where = (T, dk, w, bf, bwd)
                        assert max(out.lds_qblock, out.lds_dkv, out.lds_relgrad) <= LDS_MAX, where
                        assert (out.form == TILED) == (T > 512) and out.form in FORM, where
                        assert out.bf16 == (bf if T <= 512 else 0) and out.dk96 == (dk == 96), where
                        assert (out.lds_qblock > 0) == (T <= 512) and (out.lds_dkv > 0) == bool(bwd), where
                        if bwd and w >= 0 and T <= 512:
                            dc = out.relgrad_dc
                            assert dc > 0 and (dc % 8 == 0 or dc == dk) and dc <= dk and (2 * w + 1) * dc <= 256, where
                            assert out.relgrad_grid_y == -(-dk // dc) and out.lds_relgrad == _lds_relgrad(2 * w + 1, T, dc), where
                        else:
                            assert out.relgrad_dc == 0 and (out.lds_relgrad > 0) == bool(bwd and w >= 0), where
    m = _mirror(256, 96, 4, False, False)
    assert (m.form, m.lds_qblock) == (SHORT16, 157952)          # the shape the LDS strip was sized for still takes it
    assert _mirror(512, 128, 7, False, False).lds_qblock == 152320


def test_the_rules_before_the_plan_fail_the_sweep():
    """The launchers as they were (T <= 256: the LDS strip whatever the head width; DC = min(dk, (256 / nr) & ~7) whatever T)
    restated: the shapes at which they asked for more than 160 KiB, which the sweep above would have reported."""
    old_q = lambda dk, T: _lds_qblock(dk, T, T > 256)
    old_r = lambda dk, w, T: _lds_relgrad(2 * w + 1, T, min(dk, (256 // (2 * w + 1)) & ~7))
    first = lambda f: next(T for T in range(1, 513) if f(T) > LDS_MAX)
    assert old_q(96, 256) == 157952 <= LDS_MAX
    assert (old_q(112, 256), first(lambda T: old_q(112, T))) == (169472, 225)
    assert (old_q(128, 256), first(lambda T: old_q(128, T))) == (180992, 193)
    assert (old_r(48, 2, 512), first(lambda T: old_r(48, 2, T))) == (217472, 386)
    assert first(lambda T: old_r(80, 1, T)) == 246 and first(lambda T: old_r(96, 0, T)) == 211
    for dk, w, T in ((112, 4, 240), (128, -1, 208), (128, 7, 256), (96, 1, 256), (96, 1, 512), (48, 2, 512), (96, 0, 224)):
        m = _mirror(T, dk, w, False, True)
        assert max(m.lds_qblock, m.lds_relgrad) <= LDS_MAX < max(old_q(dk, T), old_r(dk, w, T) if w >= 0 else 0), (dk, w, T)


def test_every_branch_is_reached():
    """The labels the mirror gives the rows of CASES are exactly the branches the table is there for; one e2e row and one row with
    running sums per form; the issue's named shapes are rows."""
    got = set().union(*[_labels(c.name) for c in CASES])
    assert got == EXPECT, (sorted(EXPECT - got), sorted(got - EXPECT))
    assert len(BY_NAME) == len(CASES)
    for c in CASES:
        assert c.B <= 3 and c.H <= 3 and c.T <= 577 and c.dk % 16 == 0, c.name
    for flag in ("e2e", "start"):
        forms = sorted(FORM[_mirror(c.T, c.dk, c.w, False, True).form] for c in CASES if getattr(c, flag) and c.w >= 0)
        assert forms == sorted(FORM.values()), (flag, forms)
    shapes = {(c.T, c.dk, c.w) for c in CASES}
    assert {c.T for c in CASES} >= {1, 15, 16, 17, 63, 64, 65, 160, 161, 256, 257, 320, 512, 513, 577}
    assert {c.dk for c in CASES} >= {16, 48, 96, 112, 128} and {c.w for c in CASES} >= {-1, 0, 1, 2, 4, 7}
    assert shapes >= {(256, 96, 1), (512, 96, 1), (512, 48, 2), (224, 96, 0), (5, 16, 7)}
    assert {(c.T, c.dk) for c in CASES} >= {(240, 112), (208, 128), (256, 128), (512, 128)} and (4, 32) in {(c.w, c.dk) for c in CASES}
    assert any(c.share == 0 and c.H == 3 for c in CASES)


def test_plans_agree_with_the_mirror():
    """The library's own answer (glowtts_attn_plan_for) for every row, forward and backward, both arithmetics."""
    from glow_tts_train import _hip

    lib = _hip.load()
    for c in CASES:
        for bwd in (0, 1):
            for bf in (0, 1):
                got, want = _plan(lib, _hip, c.T, c.dk, c.w, bf, bwd), _mirror(c.T, c.dk, c.w, bf, bwd)
                assert {f: getattr(got, f) for f in _FIELDS} == {f: getattr(want, f) for f in _FIELDS}, (c.name, bwd, bf)
    out = _hip.AttnPlan()
    for dk, w, match in ((24, 2, "multiple of 16"), (144, 2, "multiple of 16"), (16, 8, "window 8")):
        assert lib.glowtts_attn_plan_for(8, dk, w, 0, 0, ctypes.byref(out)) != 0 and match in lib.glowtts_last_error().decode()
    assert lib.glowtts_attn_plan_for(0, 16, 2, 0, 1, ctypes.byref(out)) == 0 and all(getattr(out, f) == 0 for f in _FIELDS)


def test_selection_hits_every_target():
    """Over the table pi reaches: the diagonal, +-w and +-(w+1) with w > 0, the first and last key, a key of the last partial 16-tile,
    a key of another 64-key tile than the query's, both band edges under a block band; every selected pair is a kept pair."""
    hit = set()
    for c in CASES:
        pi, L = _pi(c.name), _lengths(c)
        for b in range(c.B):
            n = int(L[b])
            i = torch.arange(n)
            for h in range(c.H):
                j = pi[b, h, :n]
                assert bool(((j >= 0) & (j < n)).all()) and (c.bl < 0 or bool(((j - i).abs() <= c.bl).all())), c.name
                d = j - i
                hit.update(["diag"] if bool((d == 0).any()) else [])
                if c.w > 0:
                    hit.update(f"{s}{k}" for s, sg in (("+", 1), ("-", -1)) for k, kk in (("w", c.w), (f"w{s}1", c.w + 1)) if bool((d == sg * kk).any()))
                hit.update(["first"] if bool(((j == 0) & (i > 0)).any()) else [])
                hit.update(["last"] if bool(((j == n - 1) & (i < n - 1)).any()) else [])
                hit.update(["partial-tile"] if n % 16 and bool(((j >= n - n % 16) & (j // 16 != i // 16)).any()) else [])
                hit.update(["other-64-tile"] if bool((j // 64 != i // 64).any()) else [])
                if c.bl > 0:
                    hit.update(s for s, sg in (("+bl", 1), ("-bl", -1)) if bool((d == sg * c.bl).any()))
        assert bool((pi[:, :, :][(torch.arange(c.T)[None] >= L[:, None])[:, None, :].expand_as(pi)] == -1).all())
    assert hit == {"diag", "+w", "-w", "+w+1", "-w-1", "first", "last", "partial-tile", "other-64-tile", "+bl", "-bl"}, sorted(hit)


def test_selection_inputs_are_exact_on_the_cpu():
    """The selection inputs evaluated with the reference formulas in fp32 torch on the CPU give exactly the fp64 result, and both
    the index arithmetic of _select_expect: the inputs are exact (one-hot softmax, integer sums), whatever the kernel does; the
    same with the bf16 rounding of the operands (every value is a bf16 number)."""
    for c in CASES:
        I = _inputs(c.name, "select")
        E = _select_expect(c, I)
        lv = E.live[..., None].expand_as(E.p)
        lo = E.live[:, :, None, :].expand(c.B, c.H, c.dk, c.T).reshape(E.out.shape)
        for dt, bf in ((F64, False), (F32, False), (F32, True)):
            R = _Ref(c, I, dt, bf)
            p = R.p()[0]
            assert torch.equal(torch.where(lv, p.double(), E.p), E.p), (c.name, dt, bf)
            if bool((~lv).any()):
                assert float((p.double()[~lv] - 1.0 / c.T).abs().max()) <= U / c.T
            p_arg = torch.where(lv, E.p, torch.full((), 1.0 / c.T, dtype=F64)).float()
            out = R.out(p_arg)[0]
            assert torch.equal(torch.where(lo, out.double(), E.out), E.out), (c.name, dt, bf)
            ds = R.ds(p_arg)[0]
            assert not bool(ds.any()), (c.name, dt, bf)
            assert not bool(R.dq(ds)[0].any()) and not bool(R.dk(ds)[0].any())
            assert torch.equal(R.dv(p_arg)[0].double(), E.dv), (c.name, dt, bf)
            if c.w >= 0:
                assert torch.equal(R.demb_v(p_arg)[0].double(), E.demb_v) and not bool(R.demb_k(ds)[0].any()), (c.name, dt, bf)
        for t in (I.q, I.k, I.v, I.dout) + ((I.emb_k, I.emb_v) if c.w >= 0 else ()):
            live = I.mask.bool()[:, None, :].expand_as(t) if t.dim() == 3 and t.shape[-1] == c.T else None
            tt = t if live is None else t[live]
            assert torch.equal(tt.to(BF16).float(), tt), c.name


def test_closed_form_backward_matches_autograd():
    """The backward formulas of the module docstring against fp64 autograd of the forward ones, at two small rows with every
    feature (per-head embeddings, block band, keep bytes, ragged lengths)."""
    for name in ("T17-bl3", "T63-dc24", "T15"):
        c, I0 = BY_NAME[name], _inputs(name, "random")
        I = types.SimpleNamespace(**vars(I0))
        if I.drop is None:
            I.drop = (torch.rand(c.B, c.H, c.T, c.T, generator=_gen(name, 9)) < 0.7).to(torch.uint8)
            I.drop_scale = 2.0
        leaves = {}
        for n in ("q", "k", "v", "emb_k", "emb_v"):
            leaves[n] = getattr(I, n).double().requires_grad_(True)
            setattr(I, n, leaves[n])
        R = _Ref(c, I, F64)
        p = R.p()[0]
        Pd = torch.where(R.kb, p * I.drop_scale, torch.zeros((), dtype=F64))
        out = R.apply(Pd, I.v, R.ev)[0]
        out.backward(I.dout.double())
        J = types.SimpleNamespace(**{**vars(I), **{n: t.detach() for n, t in leaves.items()}})
        R2 = _Ref(c, J, F64)
        p32 = p.detach()
        R2.dropped = lambda _p: Pd.detach()                      # the fp64 Pd itself: no fp32 product in this comparison
        ds = R2.ds(p32)[0]
        for n, want in (("q", R2.dq(ds)[0]), ("k", R2.dk(ds)[0]), ("v", R2.dv(p32)[0]), ("emb_k", R2.demb_k(ds)[0]), ("emb_v", R2.demb_v(p32)[0])):
            g = leaves[n].grad
            assert float((g - want).abs().max()) <= 1e-12 * max(1.0, float(g.abs().max())), (name, n)


@functools.lru_cache(maxsize=None)
def _fp32_cpu_figures():
    """What plain fp32 torch on the CPU shows against fp64 on the same random inputs: per output the worst figure over CASES."""
    figs, red = {k: 0.0 for k in BOUNDS}, 0.0
    for c in CASES:
        I = _inputs(c.name, "random")
        R64, R32 = _Ref(c, I, F64), _Ref(c, I, F32)
        p_arg = _p_arg(c.name, "random")
        (p64, ps), (p32, _) = R64.p(), R32.p()
        figs["p"] = max(figs["p"], _units(p32, p64, ps))
        (ds64, dss), (ds32, _) = R64.ds(p_arg), R32.ds(p_arg)
        figs["ds"] = max(figs["ds"], _units(ds32, ds64, dss))
        ds_arg = ds64.float()
        for key, a, b in (("out", R64.out(p_arg), R32.out(p_arg)), ("dq", R64.dq(ds_arg), R32.dq(ds_arg)),
                          ("dk", R64.dk(ds_arg), R32.dk(ds_arg)), ("dv", R64.dv(p_arg), R32.dv(p_arg))):
            figs[key] = max(figs[key], _units(b[0], a[0], a[1]))
        if c.w >= 0:
            for a, b in ((R64.demb_k(ds_arg), R32.demb_k(ds_arg)), (R64.demb_v(p_arg), R32.demb_v(p_arg))):
                red = max(red, _red_fig(b[0], a[0], a[1]))
    return figs, red


def test_bound_table_matches_fp32_cpu_evaluation():
    """Every element-wise bound is 4 x the fp32-CPU figure rounded up to a power of two: fig <= bound <= 16 fig (4 x, the rounding
    to a power of two, and a factor 2 for another CPU's vector width)."""
    figs, red = _fp32_cpu_figures()
    for key, fig in sorted(figs.items()):
        print(f"fp32 CPU {key}: {fig:.2f} u (bound {BOUNDS[key]})")
    print(f"fp32 CPU reductions: {red:.1e} of sum|term| (the bound {RED:.0e} is the project's figure for block sums + atomics)")
    assert red <= RED
    for key, fig in figs.items():
        bound = BOUNDS[key]
        assert bound == 2 ** round(math.log2(bound)), key
        assert fig <= bound <= 16 * fig, (key, fig, bound)
