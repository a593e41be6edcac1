// conv_plan.hpp — how a launch of the convolution family is chosen (host only): convgemm.hip, convgemm_split.hip, convwrw_tr.hip and the
// two hooks of convwino.hip.  An entry point checks its arguments, fills the kernel's parameter block, PLANS (plan_conv_fwd /
// plan_conv_wrw: pure functions of the block and a ConvSnapshot — no HIP call, no allocation, nothing formatted) and LAUNCHES the plan
// (launch_conv_fwd / launch_conv_wrw: per family ONE ladder from plan fields to a template instantiation, then launch_planned).  Every
// rule the decision is made of is ONE function below, with the measurement it came from.  glowtts_conv_plan_next (include/glowtts_hip.h)
// hands the plan to the caller instead of launching it, so the decision is testable without a GPU (tests/test_conv_kernels.py).
#pragma once
#include "convgemm_common.hpp"

namespace glowtts {

using ConvPlan = glowtts_conv_plan;

// What a decision depends on besides the parameter block, taken once per call (conv_snapshot, convgemm_split.hip)
struct ConvSnapshot {
    int math_fwd, math_wrw;               // the two arithmetic modes (glowtts_conv_math)
    int bound_ns;                         // planes per value bound to this thread for the packed weights (0 = none), and where
    const unsigned short *planes;
    long plane_stride;
    const unsigned short *wino_u;         // Winograd U planes bound to this thread for the packed weights, or null
    long wino_stride;
    int cus;                              // compute units of the current device (weight gradients in a plane mode; else 0)
    int knob[K_COUNT];                    // the tuning switches the planners read (conv_snapshot lists them), latched as ever
};
ConvSnapshot conv_snapshot(const float *wp, bool wino, bool wrw);

// ---- the rules ------------------------------------------------------------------------------------------------------------------
static inline int round_up(int n, int m) { return (n + m - 1) / m * m; }

// forward-type kernels: 80-frame tiles when T divides evenly (e.g. T' = 400), else 64 unless 80 wastes less
static inline bool frames80_fwd(int T) { return (T % 80 == 0) || (T % 64 != 0 && round_up(T, 80) < round_up(T, 64)); }
// frame-packed weight gradients: 80-frame chunks, or 64 when that wastes less.  (Where both waste the same — T = 300: 320 either way —
// this rule takes 80 and the forward one 64.  Nothing was measured there; kept as found.)
static inline bool frames80_wrw(int T) { return (T % 80 == 0) || round_up(T, 80) <= round_up(T, 64); }

// 128-row workgroups unless M is small
static inline bool rows_big(int epi, int M) { return (epi == EPI_GATE) || (M % 128 == 0) || M > 192; }

// the pipelined forward-type kernels: 16-byte rows and a halo of at most 12 frames
static inline bool fwd_pipe_ok(const ConvGemmParams &p, int epi) {
    return (p.T % 4 == 0) && aligned16(p.x) && (p.x_bs % 4 == 0) && (!p.mask_in || aligned16(p.mask)) && ((p.taps - 1) * p.dil <= 12) &&
           (epi != EPI_GATE || p.H % 4 == 0);
}

// Small problems (the text encoder: T = 160) give only ~190 workgroups with 80-frame tiles — less than one per CU.
// 32-frame tiles fill the chip (480+ workgroups): -15..20 % on the encoder's 3-tap and 1-tap convs.  At the decoder's
// T' = 400 (480 workgroups already) the smaller tiles only lose operand reuse, so the switch is on the grid size.
static inline bool fwd_use32(const ConvGemmParams &p, int epi, bool big, bool pipe_ok, int conv32_1x1) {
    if (epi != EPI_PLAIN || !pipe_ok) return false;
    const int rows_per = big ? 128 : 64;
    const long wg5 = (long)((p.T + 79) / 80) * p.B * ((p.M + rows_per - 1) / rows_per);
    const int t32 = round_up(p.T, 32);
    // (threshold 440 -> 380 in round 4: the FFN's 768 <- 192-channel 3-tap convolutions at T = 160 have 384 tiles of 128 rows
    // x 80 frames, which the bf16-plane kernel runs in 80-frame form — its 32-frame 128-row form does not exist, and the native
    // 32-frame kernel that served them took 49 us: 15.00 -> 14.81 ms per step, tools/ab_flags.py envs=GLOWTTS_CONV32_WG:440,..:380;
    // 190 and 0 measured 14.87 / 14.96 against 14.90)
    if (wg5 < 380 && t32 * 10 <= p.T * 11) return true;
    // plain 1x1 convolutions (the coupling's start / end convs and the end conv's backward-data: 12 800 columns, 480 tiles of
    // 80 frames) take 32-frame tiles as well: four consecutive A/B pairs 15.04 -> 15.00 ms per step (GLOWTTS_CONV32_1X1=0 / 1)
    return p.taps == 1 && t32 * 10 <= p.T * 11 && conv32_1x1 == 1;
}

// 16-byte epilogue through LDS: every tensor the epilogue touches has 16-byte rows.  (The bf16-plane kernels do not look at gate_pos,
// which their vector epilogue reads 16 bytes at a time as well; the Python host only ever passes whole tensors there.  Kept as found.)
static inline bool vec_epilogue(const ConvGemmParams &p, int epi, bool native) {
    return aligned16(p.y0) && aligned16(p.y1) && aligned16(p.r0) && aligned16(p.r1) && aligned16(p.mask) && aligned16(p.drop) &&
           (!native || aligned16(p.gate_pos)) && (p.y_bs % 4 == 0) && (p.r_bs % 4 == 0) && (epi != EPI_GATE || p.H % 4 == 0);
}

// the forward-type workgroup grid: frame tiles x utterances, row tiles (the gate: 64 channels of each half per workgroup)
static inline void fwd_grid(const ConvGemmParams &p, ConvPlan &plan) {
    const int rows = (plan.epi == EPI_GATE) ? p.H : p.M;
    const int per = (plan.epi == EPI_GATE) ? 64 : plan.rows;
    plan.grid_x = ((p.T + plan.frame_tile - 1) / plan.frame_tile) * p.B;
    plan.grid_y = (rows + per - 1) / per;
    plan.grid_z = 1;
}

// Split-K of a weight gradient: the contraction's `total` items go to `splits` workgroups per tile, plan.nb items each.  The callers
// pass splits = slots / tiles so that ALL workgroups are resident at once (a grid of 576 on 512 slots costs two full rounds).
static inline void wrw_split_k(ConvPlan &plan, int tiles, int total, int splits) {
    if (splits > total) splits = total;
    if (splits < 1) splits = 1;
    plan.nb = (total + splits - 1) / splits;
    plan.grid_x = tiles;
    plan.grid_y = 1;
    plan.grid_z = ((total + plan.nb - 1) / plan.nb) * (plan.nbatch > 0 ? plan.nbatch : 1);
}

// 16-byte rows of both operands (of every problem of a batch) and a halo of at most 12 frames
static inline bool wrw_pipe_ok(const ConvWrwParams &p) {
    bool ok = (p.T % 4 == 0) && (p.x_bs % 4 == 0) && (p.d_bs % 4 == 0) && (!p.mask || aligned16(p.mask)) &&
              (!p.mask_x || aligned16(p.mask_x)) && ((p.taps - 1) * p.dil <= 12) && (!p.d2 || (p.d2_bs % 4 == 0 && p.d_split % 64 == 0));
    if (p.nbatch > 0)
        for (int q = 0; q < p.nbatch; ++q) ok = ok && aligned16(p.bx[q]) && aligned16(p.bd[q]) && aligned16(p.bd2[q]);
    return ok && aligned16(p.x) && aligned16(p.d) && aligned16(p.d2);
}
// ... and what the frame-packed kernels (fp32, bf16 planes, transposed-read) take: 1 / 3 / 5 taps, dilation 1, 'same' padding
static inline bool wrw_frame_packed(const ConvWrwParams &p) {
    return wrw_pipe_ok(p) && (p.taps == 1 || p.taps == 3 || p.taps == 5) && p.dil == 1 && p.pad == (p.taps - 1) / 2;
}
// 5 taps: 64 k x 32 m tiles — 40 accumulator registers per lane instead of 80, so THREE workgroups fit a CU (168
// VGPRs, 36 KB LDS) and hide each other's prologue / atomics epilogue: 107 -> 96 us at config 2.  With 3 taps or 1 the
// 64 x 64 tile already leaves room for three, and the smaller tile only costs operand reuse.
static inline int wrw_fp_mt(const ConvWrwParams &p) {
    return (p.taps == 5 && p.M % 32 == 0 && (!p.d2 || p.d_split % 32 == 0)) ? 2 : 4;
}

// ---- dynamic LDS of the kernels (the launch ladders static_assert the occupancy they were tuned for on the same formulas) ---------
constexpr int cpitch2(int n) { return ((n - 2 + 31) / 32 * 32 + 2) < n ? ((n - 2 + 31) / 32 * 32 + 2) + 32 : ((n - 2 + 31) / 32 * 32 + 2); }
__host__ __device__ constexpr int cpitch4(int w) { int p = (w + 3) / 4 * 4; while (p % 8 != 4) p += 4; return p; }
static inline int pitch16(int n) {          // smallest pitch >= n with pitch % 32 == 16
    int p = (n + 15) / 32 * 32 + 16;
    if (p - 32 >= n) p -= 32;
    return p;
}
constexpr size_t lds_max(size_t a, size_t b) { return a > b ? a : b; }
constexpr size_t lds_epilogue(int wgr, int nt, int epi) { return ((size_t)wgr * (nt + 4) + (epi == EPI_GATEBWD ? 2 * wgr : 0)) * sizeof(float); }
constexpr size_t lds_conv_pipe(int wgr, int nt, int epi) {
    return lds_max(((size_t)6 * (nt + 16) * 20 + (nt + 16)) * sizeof(float), lds_epilogue(wgr, nt, epi));
}
constexpr size_t lds_conv_split(int ns, int wgr, int nt, int epi) {
    return lds_max((size_t)ns * 3 * (nt + 16) * 80 + (size_t)(nt + 16) * sizeof(float), lds_epilogue(wgr, nt, epi));
}
constexpr size_t lds_wrw_fp(int ct, int mr) { return ((size_t)64 * cpitch4(ct + 16) + (size_t)mr * cpitch4(ct) + (ct + 16) + ct) * sizeof(float); }
constexpr size_t lds_wrw_pipe(int ct) { return 2 * ((size_t)64 * cpitch2(ct + 16) + (size_t)64 * cpitch2(ct)) * sizeof(float); }
constexpr size_t lds_wrw_split(int ns, int ct, int mr) { return (size_t)ns * (64 + mr) * 104 * 2 + (size_t)(ct + 8 + ct + 64) * sizeof(float); }

// ---- plan -> launch ----------------------------------------------------------------------------------------------------------------
// The one place a planned kernel is launched: its LDS limit (per device: raised only when a launch needs more than any earlier
// one), the plan's grid, block and LDS bytes.
template <auto Kernel, class... Args>
static int launch_planned(const ConvPlan &plan, const char *who, hipStream_t s, Args... args) {
    static LdsLimit attr_max_e;
    if (int rc_ = attr_max_e.ensure(reinterpret_cast<const void *>(Kernel), (size_t)plan.lds_bytes, who)) return rc_;
    hipLaunchKernelGGL(Kernel, dim3(plan.grid_x, plan.grid_y, plan.grid_z), dim3(plan.block), (size_t)plan.lds_bytes, s, args...);
    GLOWTTS_LAUNCH_CHECK(who);
}

// The calling thread's glowtts_conv_plan_next pointer, taken (and so disarmed) by the entry point that is about to launch: the plan
// goes to it instead of to the device.  One thread-local pointer test per call.
extern thread_local ConvPlan *t_conv_plan_out;
static inline ConvPlan *conv_plan_take() {
    ConvPlan *out = t_conv_plan_out;
    if (out) { t_conv_plan_out = nullptr; out->family = GLOWTTS_PLAN_NONE; out->launches = 0; }
    return out;
}

// convgemm.hip: the two planners; plan + launch of one weight-gradient problem (or of a batch as ONE launch) — with `dry` the plan is
// handed over instead (the first one; the launches of later ones are added to it)
int plan_conv_fwd(const ConvGemmParams &p, int epi, const ConvSnapshot &sn, ConvPlan &plan);
int plan_conv_wrw(const ConvWrwParams &p, int planes_ns, const ConvSnapshot &sn, ConvPlan &plan);
int conv_wrw_go(ConvWrwParams &p, int planes_ns, hipStream_t s, ConvPlan *dry);

// convgemm_split.hip: which bf16-plane / bf16-tensor forward kernels exist (rows = 64 or 128, nt = frame tile), their ladder, and the
// ladder of the frame-packed bf16-plane weight gradients (GLOWTTS_PLAN_WRW_SPLIT / _PLANES)
bool conv_split_has(int ns, int epi, int rows, int taps, int nt);
bool conv_bf16_has(int iob, int epi, int rows, int taps);
int launch_conv_split(ConvGemmParams &p, const ConvPlan &plan, const ConvSnapshot &sn, hipStream_t s);
int launch_wrw_split(ConvWrwParams &p, const ConvPlan &plan, hipStream_t s);

// convwrw_tr.hip: the transposed-read weight gradient; false = not for this problem (other taps, M % 32, GLOWTTS_WRW_TR=0)
int compute_units();
bool plan_wrw_tr(const ConvWrwParams &p, const ConvSnapshot &sn, ConvPlan &plan);
int launch_wrw_tr(ConvWrwParams &p, const ConvPlan &plan, hipStream_t s);

// convwino.hip: the gated 5-tap in-conv and its backward-data in Winograd F(4, 5) form from U planes bound to the calling thread;
// false = not for this problem.  launch_wino_bwd returns -1 where its workspace cannot be had (a first launch under stream capture).
void conv_wino_bound(const float *wp, const unsigned short **U, long *stride);
bool plan_wino_gate(const ConvGemmParams &p, const ConvSnapshot &sn, ConvPlan &plan);
bool plan_wino_bwd(const ConvGemmParams &p, const ConvSnapshot &sn, ConvPlan &plan);
int launch_wino_gate(ConvGemmParams &p, const ConvPlan &plan, const ConvSnapshot &sn, hipStream_t s);
int launch_wino_bwd(ConvGemmParams &p, const ConvPlan &plan, const ConvSnapshot &sn, hipStream_t s);

}  // namespace glowtts
