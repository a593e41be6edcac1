// flow_plan.hpp — how a launch of the flow family is chosen (host only): the entry points of flows.hip.
// Each of them checks its arguments, PLANS (plan_flow: a pure function of the operation, the shape, n_split, the direction and
// the alignment verdict — no HIP call, nothing formatted) and launches what the plan says; every grid rule of the family is one
// function here, with the measurement it came from, and exists nowhere else.  glowtts_flow_plan_for (include/glowtts_hip.h) hands
// the plan to the caller, so the decision is testable without a GPU (tests/test_flow_kernels.py).
#pragma once
#include "glowtts_hip.h"

namespace glowtts {

using FlowPlan = glowtts_flow_plan;

static inline long flow_cdiv(long a, long b) { return (a + b - 1) / b; }

// the group sizes whose n x n mix is held in registers (invconv_fwd_kernel / invconv_bwd_kernel<N, V>); every other even
// n_split <= 32 runs on the run-time-N kernels
static inline bool flow_register_n(int n_split) { return n_split == 2 || n_split == 4 || n_split == 8; }

// actnorm_bwd, actnorm_stats (grid (C, slabs of utterances)): utterances per workgroup row — enough workgroups to fill 256 CUs
// several times over, at least one utterance per workgroup
static inline int flow_slab_size(int B, int C) {
    int nbk = (2048 + C - 1) / C;
    if (nbk > B) nbk = B;
    if (nbk < 1) nbk = 1;
    return (B + nbk - 1) / nbk;
}

// actnorm_invconv_bwd, coupling_actnorm_invconv_bwd (grid (G, slabs of items)): slabs = min(ceil(200 / G), ceil(items / 256)), at
// least 1: ~200 workgroups, and no more slabs than give every thread an item (see the comment of actnorm_invconv_bwd_kernel).
// Measured on actnorm_invconv_bwd at B=32, C=160, T=400: 80 / 120 / 160 / 200 / 288 / 400 / 520 workgroups take 10.9 / 9.5 / 9.1 /
// 8.9 / 9.6 / 10.6 / 11.7 us; on coupling_actnorm_invconv_bwd, 120 .. 800 workgroups: 200 is the fastest, 13.2 us at config 2.
// -> nb = items per slab; *slabs = the slabs that hold an item (grid.y)
static inline int flow_fused_bwd_nb(int G, long items, int *slabs) {
    long want = (200 + G - 1) / G;
    if (want > flow_cdiv(items, 256)) want = flow_cdiv(items, 256);
    if (want < 1) want = 1;
    const long nb = flow_cdiv(items, want);
    *slabs = (int)flow_cdiv(items, nb);
    return (int)nb;
}

// Workgroups per utterance (grid.x of the kernels with grid (x, B), which walk an utterance's items in a grid-stride loop).
//   coupling forward 16    : one logdet[b] atomic per workgroup, same cache line for 16 b
//   coupling reverse 64, coupling backward 64 : no atomic
//   coupling o ActNorm/InvConv forward 8 : one logdet_prev[b] atomic per workgroup; 8 x B workgroups of ~2 items per thread:
//                            7.3 us at config 2 where 16 x B (one item per thread) took 8.9
static inline int flow_utterance_cap(int op, bool reverse) {
    switch (op) {
    case GLOWTTS_FLOW_COUPLING_FWD: return reverse ? 64 : 16;
    case GLOWTTS_FLOW_COUPLING_BWD: return 64;
    default: return 8;                     // GLOWTTS_FLOW_COUPLING_ACTNORM_INVCONV_FWD
    }
}

// Grid caps of the flat kernels that end in atomics or keep per-workgroup state, which walk their items in a grid-stride loop:
// invconv_bwd_kernel 1024 (every workgroup ends in n^2 atomics on one cache line), invconv_mix_generic_kernel 4096 (each
// workgroup stages W in LDS first).
static inline int flow_grid_cap(bool register_n) { return register_n ? 1024 : 4096; }

static inline int flow_capped(long items, int cap) {
    const long g = flow_cdiv(items, 256);
    return (int)(g > cap ? cap : g);
}

// The arguments are checked by the caller (flow_check in flows.hip); B, C, T > 0.  aligned: every tensor the vector kernels touch
// is 16-byte aligned (all_aligned16 over the entry point's own list).
static inline FlowPlan plan_flow(int op, int B, int C, int T, int n_split, bool reverse, bool aligned) {
    FlowPlan pl{};
    pl.width = aligned && T % 4 == 0 ? 4 : 1;
    pl.launches = 1;
    pl.grid_y = 1;
    const long TV = T / pl.width;
    switch (op) {
    case GLOWTTS_FLOW_ACTNORM_FWD:                              // thread -> (b, c, t-vector)
        pl.grid_x = (int)flow_cdiv((long)B * C * TV, 256);
        break;
    case GLOWTTS_FLOW_ACTNORM_BWD:
    case GLOWTTS_FLOW_ACTNORM_STATS:
        pl.nb = flow_slab_size(B, C);
        pl.grid_x = C;
        pl.grid_y = (B + pl.nb - 1) / pl.nb;
        break;
    case GLOWTTS_FLOW_INVCONV_FWD:
    case GLOWTTS_FLOW_INVCONV_BWD: {
        const bool bwd = op == GLOWTTS_FLOW_INVCONV_BWD;
        if (flow_register_n(n_split)) {                         // thread -> (b, group, t-vector)
            pl.n = n_split;
            const long items = (long)B * (C / n_split) * TV;
            pl.grid_x = bwd ? flow_capped(items, flow_grid_cap(true)) : (int)flow_cdiv(items, 256);
        } else {                                                // thread -> (b, c, t-vector); backward: dx = W^T (dz mask), then dW
            pl.grid_x = flow_capped((long)B * C * TV, flow_grid_cap(false));     // entry by entry
            if (bwd) { pl.launches = 2; pl.grid2_x = n_split * n_split; }
        }
        break;
    }
    case GLOWTTS_FLOW_ACTNORM_INVCONV_FWD:                      // thread -> (b, group, t-vector)
        pl.n = n_split;
        pl.grid_x = (int)flow_cdiv((long)B * (C / n_split) * TV, 256);
        break;
    case GLOWTTS_FLOW_ACTNORM_INVCONV_BWD:
    case GLOWTTS_FLOW_COUPLING_ACTNORM_INVCONV_BWD:
        pl.n = n_split;
        pl.grid_x = C / n_split;
        pl.nb = flow_fused_bwd_nb(pl.grid_x, (long)B * TV, &pl.grid_y);
        break;
    case GLOWTTS_FLOW_COUPLING_FWD:
    case GLOWTTS_FLOW_COUPLING_BWD:                             // grid (x, B): thread -> (c < C/2, t-vector) of utterance b
        pl.grid_x = flow_capped((long)(C / 2) * TV, flow_utterance_cap(op, reverse));
        pl.grid_y = B;
        break;
    case GLOWTTS_FLOW_COUPLING_ACTNORM_INVCONV_FWD:             // grid (x, B): thread -> (group, t-vector) of utterance b
        pl.n = n_split;
        pl.grid_x = flow_capped((long)(C / n_split) * TV, flow_utterance_cap(op, reverse));
        pl.grid_y = B;
        break;
    }
    return pl;
}

}  // namespace glowtts
