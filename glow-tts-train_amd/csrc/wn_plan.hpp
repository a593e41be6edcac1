// wn_plan.hpp — how the backward of a WN stack is queued (host only): glowtts_wn_bwd_io and glowtts_flow_block_bwd_io of
// wn_stack.hip.  Both check their arguments, PLAN (plan_wn_bwd: a pure function of the stack's shape, what the caller asks for,
// who the caller is and the WRW_BATCH switch — no HIP call, nothing formatted) and queue what the plan says; the two-source shape
// rule and the limit of the local operand tables are stated here and nowhere else.  glowtts_wn_bwd_plan_for
// (include/glowtts_hip.h) hands the plan to the caller: convops.py sizes the d_rs workspace from it, and the decision is testable
// without a GPU (tests/test_wn_executor.py).
#pragma once
#include "glowtts_hip.h"

namespace glowtts {

using WnBwdPlan = glowtts_wn_bwd_plan;

// Problems per local operand table: the executor's tables for glowtts_conv_wrw_batch (one entry per layer) and the block's
// glowtts_wrw1_problem table (one entry per layer, the end conv, the start conv: one launch of glowtts_conv_wrw1_multi holds 8).
// A stack with more layers takes the per-layer order / the stack's own 1x1 launches.
constexpr int kWnTableMax = 8;

// The two-source form (d_rs = [dx_{i+1} mask ; dskip] is never written: conv_gate_bwd and conv_wrw2 read its halves from the two
// tensors) needs fp32 tensors, unit dilation, whole 96-channel chunks per source in the frame-packed weight-gradient kernel and
// 16-byte rows.
static inline bool wn_two_source_shape(int io, int dil_rate, int H, int T) {
    return !io && dil_rate == 1 && H % 192 == 0 && T % 4 == 0;
}

// two_source: the argument of glowtts_wn_bwd(_io) — bit 0 the form, bit 1 (with bit 0) `dskip` arrives masked, bit 2 (with bits 0
// and 1) the caller queues the stack's 1x1 weight gradients itself — or, in_block, glowtts_flow_block_bwd(_io)'s: non-zero asks for
// the form, and the block masks dskip in the end conv's backward-data epilogue.  The arguments are checked by the caller
// (wn_bwd_check in wn_stack.hip): a two-source plan exists only where wn_two_source_shape holds.
static inline WnBwdPlan plan_wn_bwd(int n_layers, int B, int H, int T, int dil_rate, int io, int two_source, bool in_block,
                                    bool wrw_batch) {
    WnBwdPlan pl{};
    const int n = n_layers;
    pl.two_source_ok = wn_two_source_shape(io, dil_rate, H, T);
    pl.two_source = in_block ? two_source != 0 : (two_source & 1);
    if (!pl.two_source) {
        // the whole dx chain first (res_skip_bwd, conv_gate_bwd, conv_fwd per layer), then both weight gradients of every layer
        pl.wrw_order = GLOWTTS_WN_WRW_AFTER_CHAIN;
        pl.d_rs_elems = (int64_t)n * B * 2 * H * T;
        pl.chain_calls = 3 * n;
        pl.wgrad_calls = 2 * n;
        return pl;
    }
    pl.pre_masked = in_block || (two_source & 2);
    // the block's 1x1 weight gradients (the stack's, the end conv's, the start conv's) as ONE glowtts_conv_wrw1_multi launch
    pl.block_wrw1 = in_block ? n + 2 <= kWnTableMax && H % 64 == 0 : pl.pre_masked && (two_source & 4);
    pl.wrw_order = wrw_batch && n <= kWnTableMax ? GLOWTTS_WN_WRW_BATCHED : GLOWTTS_WN_WRW_PER_LAYER;
    pl.d_rs_elems = (int64_t)B * H * T;                  // the last layer's masked dskip
    pl.chain_calls = 2 * n + (pl.pre_masked ? 0 : 1);    // conv_gate_bwd, conv_fwd per layer; res_skip_bwd of the last layer
    // batched: the 5-tap problems in one launch, the last layer's 1x1 alone, the two-source 1x1 ones of layers 0 .. n-2 in another
    const int wrw1 = pl.block_wrw1 ? 0 : pl.wrw_order == GLOWTTS_WN_WRW_BATCHED ? 1 + (n > 1) : n;
    pl.wgrad_calls = (pl.wrw_order == GLOWTTS_WN_WRW_BATCHED ? 1 : n) + wrw1;
    return pl;
}

}  // namespace glowtts
