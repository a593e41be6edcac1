// attn_plan.hpp — how a launch of the relative-position attention is chosen (host only): attention.hip and attention_long.hip.
// glowtts_rel_attn_fwd_ex / _bwd_ex check their arguments, PLAN (plan_attn: a pure function of T, d_k, the window, the arithmetic and
// the direction — no HIP call, nothing formatted) and launch what the plan says; every LDS formula of the family exists here and
// nowhere else.  glowtts_attn_plan_for (include/glowtts_hip.h) hands the plan to the caller, so the decision is testable without a
// GPU (tests/test_attention_kernels.py sweeps the whole envelope the header promises).
#pragma once
#include <stddef.h>
#include "glowtts_hip.h"

namespace glowtts {

using AttnPlan = glowtts_attn_plan;

constexpr int kAP = 80;    // LDS pitch of the [d][64 queries] A block          (== 16 mod 32)
constexpr int kBP = 68;    // LDS pitch of the [d][64 keys] B tile              (==  4 mod 32)
constexpr int kCP = 68;    // LDS pitch of a wave's [16][64] probability chunk (strip-in-registers form)
constexpr int kAttnStripMaxT = 512;              // beyond: the tiled kernels of attention_long.hip
constexpr size_t kAttnLdsMax = 160 * 1024;       // dynamic LDS a workgroup can have on gfx950

// LDS pitch of the probability strip / of the strip's keep bytes
static inline int attn_tp(int T) { return ((T + 15) / 16) * 16 + 4; }

// attn_qblock_kernel: A block, B tile, the strip (strip-in-registers form: four [16][kCP] chunks and four [16][16] band tables),
// both embedding tables, the R tables, and the keep bytes of the strip
static inline size_t attn_lds_qblock(int dk, int T, bool strip_in_regs) {
    const int TP = attn_tp(T);
    const size_t strip = strip_in_regs ? (size_t)4 * 16 * kCP + 4 * 16 * 16 : (size_t)64 * TP;
    return ((size_t)dk * kAP + (size_t)dk * kBP + strip + (size_t)16 * (dk + 4) + (size_t)16 * (dk + 16) + 4 * 16 * 17) *
               sizeof(float) + (size_t)64 * TP;
}
// attn_dkv_kernel: dO and Q chunks [dk][kBP], Pd and dS chunks [64][kAP]
static inline size_t attn_lds_dkv(int dk) { return ((size_t)2 * dk * kBP + (size_t)2 * 64 * kAP) * sizeof(float); }
// attn_relgrad_kernel: the 2w+1 diagonals of Pd and dS [nr][T], the slab's dO and Q rows [DC][T + 1]
static inline size_t attn_lds_relgrad(int nr, int T, int DC) { return ((size_t)2 * nr * T + (size_t)2 * DC * (T + 1)) * sizeof(float); }
// attn_long_relgrad_kernel (tiled form): one diagonal of Pd or dS
static inline size_t attn_lds_diag(int T) { return (size_t)T * sizeof(float); }

// channels per slab of attn_relgrad_kernel: one (r, d) output per thread ((2w+1) DC <= 256), a multiple of 8, at most d_k, and the
// slab fits LDS.  (Until the slab was capped the rule was min(dk, (256 / nr) & ~7) alone, sized for T <= 256 at window 4: window 2
// with dk >= 48 went over the limit from T = 386, window 1 with dk >= 80 from T = 246, window 0 with dk = 96 from T = 211.)  The
// smallest slab, 8 channels, fits at every T <= 512 and window <= 7: 4 (2 * 15 * 512 + 2 * 8 * 513) = 155 712 B.
static inline int attn_relgrad_dc(int nr, int T, int dk) {
    int DC = (256 / nr) & ~7;
    if (DC > dk) DC = dk;
    while (DC > 8 && attn_lds_relgrad(nr, T, DC) > kAttnLdsMax) DC = (DC - 1) & ~7;
    return DC;
}

// w: the window, or -1 without relative embeddings.  The arguments are checked by the caller (attn_check).
static inline AttnPlan plan_attn(int T, int dk, int w, bool bf16_mma, bool backward) {
    AttnPlan pl{};
    const bool rel = w >= 0;
    pl.dk96 = dk == 96;
    if (T > kAttnStripMaxT) {
        // plain tiled kernels (static LDS only, but for the diagonal of attn_long_relgrad_kernel: one workgroup per offset r and no
        // channel slab, relgrad_dc = 0); fp32 FMA whatever bf16_mma says
        pl.form = GLOWTTS_ATTN_TILED;
        pl.launches = 3;
        if (backward && rel) { pl.lds_relgrad = (int)attn_lds_diag(T); pl.relgrad_grid_y = 2 * w + 1; pl.launches += 2; }
    } else {
        // T <= 160: the strip in 10 accumulator tiles, T <= 256: in 16, both with the probability strip in LDS.  That strip was sized
        // for d_k = 96 at T = 256 (157 952 B); d_k = 112 does not fit from T = 225 and d_k = 128 from T = 193.  Those shapes take the
        // strip-in-registers form written for 256 < T <= 512 (152 320 B at d_k = 128, T = 512, so it fits wherever it is asked
        // for) rather than the tiled kernels: every loop of attn_qblock_kernel<.., LONG = true> over the strip is guarded by
        // `t < ntile` / `jt < njt` and its LDS chunk, band table and HBM reads of P are indexed by the tile at hand, so nothing in it
        // needs more than 16 tiles to be present, and it keeps the MFMA arithmetic (and the bf16_mma switch) of its neighbours.
        pl.bf16 = bf16_mma;
        pl.launches = 1;
        const bool lds_strip = T <= 256 && attn_lds_qblock(dk, T, false) <= kAttnLdsMax;
        pl.form = !lds_strip ? GLOWTTS_ATTN_STRIP32 : T <= 160 ? GLOWTTS_ATTN_SHORT10 : GLOWTTS_ATTN_SHORT16;
        pl.lds_qblock = (int)attn_lds_qblock(dk, T, !lds_strip);
        if (backward && rel) {
            const int nr = 2 * w + 1;
            pl.relgrad_dc = attn_relgrad_dc(nr, T, dk);
            pl.relgrad_grid_y = (dk + pl.relgrad_dc - 1) / pl.relgrad_dc;
            pl.lds_relgrad = (int)attn_lds_relgrad(nr, T, pl.relgrad_dc);
            pl.launches += 1;
        }
    }
    if (backward) { pl.lds_dkv = (int)attn_lds_dkv(dk); pl.launches += 1; }
    return pl;
}

}  // namespace glowtts
