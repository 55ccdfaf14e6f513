// Which kernel runs a conv flow step (host only): Kernel, Pass, the batch thresholds and select().  Included by every unit that
// launches a step kernel of the forward (cf_step_tile.h, cf_step_small.h, cf_step_rs.h) or inverse (cf_step_inv.h) families -
// cf_step.hip and cf_step_inv_ctx.hip ask the same select().
#pragma once
#include "cf_step_common.h"
#include <atomic>
#include <cstdlib>

static bool direct_conv_only() {
    static const bool v = [] { const char* e = getenv("CONTEXTFLOW_DIRECT_CONV"); return e && e[0] == '1'; }();
    return v;
}
// ---- dispatch: the ONE place that says which kernel runs a step ---------------------------------------------------------
// A kernel family with its geometry, one value per pair the library launches outside the test hook's alternates.
enum class Kernel {
    None,
    Small_G8s, Small_G16s, Small_G8w, Small_G16w,                                                                  // k_flow_step_small
    Step_G8, Step_G16, Step_G32, Step_G32v2, Step_G32w, Step_G32w24, Step_G64, Step_G64v2, Step_G64w2, Step_G64w24,   // k_flow_step
    Step_G64z24,                                                                                                   // ... on 8 waves
    Rs_G32,                                                                                                        // k_flow_step_rs<.., 2>
    Rs16_G64,                                                                                                      // k_flow_step_rs16
    Inv_G8, Inv_G8w, Inv_G16, Inv_G16w, Inv_G32, Inv_G32w, Inv_G64, Inv_G64w2,                                     // k_flow_step_inv
};
// CtxDirect: cf_flow_step_fwd_ctx with mode | 4; Chain: cf_flow_step_fwd_chain (the kernel whose chained form runs);
// InverseCtx: cf_flow_step_inv_ctx (cf_step_inv_ctx.hip)
// Level: cf_flow_step_fwd_level (Eval's kernel among those that have a level form)
enum class Pass { Eval, Taped, Ctx, CtxDirect, CtxTaped, Chain, Inverse, InverseCtx, Level };

// Batch thresholds.  Small batches are latency-bound by the serial work of ONE workgroup (a launch of < 256 workgroups leaves CUs
// idle anyway): below these, the geometry with half the samples per workgroup (same packed-weight workspace) ...
constexpr int kFullMinB8x8 = 256 * G32::SPW;         // (also where the 8x8 level's 3x3 takes the Winograd F(2x2, 3x3) form)
constexpr int kFullMinB4x4 = 256 * G64::SPW;
// ... 4x4: 8 samples per workgroup, rows split over wave pairs (F(2x2)) / over all four waves (F(2x4), 24 instead of 32 products per 8 pixels)
constexpr int kWinoMinB4x4 = 256 * G64w2::SPW;
// smallest batch of the 8x8 level's F(2x4) form: 512 workgroups = one full round of 2 per CU, as at 4x4 (below: F(2x2), G32w)
constexpr int kW24MinB8x8 = 512 * G32w24::SPW;
// 4x4, evaluation: from here the F(2x4) form with 16 samples on 8 waves, which skips the products reflection zeroes (G64z24).  The
// smallest size of the ladder 4 096 .. 262 144 at which it beat G64w24 by more than 5x that kernel's run-to-run spread (it is 10 %
// faster from 4 096 on, but the spread of these sub-millisecond launches hides that up to 16 384: profiles/w24_zero_skip.md); above
// every batch at which a test pins the kernel.  The switch is on in every default path; A/B runs and tests turn it off through the
// hook cf_flow_step_zero_skip_enable (one flag per process, so that one process can run both)
constexpr int kZeroSkipMinB4x4 = 65536;
inline std::atomic<bool> g_zero_skip{true};
static bool zero_skip_enabled() { return g_zero_skip.load(std::memory_order_relaxed); }
// very small batches: the row-split kernel (a quarter of the serial chain per workgroup, 4x the workgroups)
constexpr int kRsMaxB8x8 = 512;
// 4x4: one sample per workgroup on 16-column tiles (twice the workgroups of the row-split kernel) up to here, Winograd above
constexpr int kRs16MaxB4x4 = 1024;
// 16x16 images: chained launches (cf_flow_step_fwd_chain) up to here
constexpr int kChainMaxB16x16 = 1024;

// largest batch cf_flow_step_fwd_chain takes: the range in which a step is one of the small-batch kernels anyway
static int chain_max_batch(int sid) {
    switch (sid) {
        case 0: case 1: return direct_conv_only() ? 0 : kChainMaxB16x16;
        case 2: return kRsMaxB8x8;
        case 3: return kRs16MaxB4x4;
    }
    return 0;
}

// The kernel of one step.  Winograd F(2x2,3x3) form of the 3x3 (winograd_phase2): 40 instead of 80 C^2 HW multiply-adds per sample
// and step; CONTEXTFLOW_DIRECT_CONV=1 keeps the direct form (A/B measurements, tools/step_bench.py), and so does CtxDirect - the
// TRAINING forward under contextflow, whose backward (cf_flow_step_bwd_ctx) rebuilds the conditioner in that form.
static Kernel select(Pass pass, int sid, int B) {
    const bool direct = direct_conv_only() || pass == Pass::CtxDirect;
    const bool eval = pass == Pass::Eval || pass == Pass::Level, ctx = pass == Pass::Ctx || pass == Pass::CtxDirect;
    if (pass == Pass::Inverse || pass == Pass::InverseCtx) {      // the conditioner is the forward's: Winograd form of its 3x3 at every
        const bool ictx = pass == Pass::InverseCtx;               // batch size.  InverseCtx: whatever CONTEXTFLOW_DIRECT_CONV says, and the
        const bool d = direct && !ictx;                           // direct geometry at C = 8, whose Winograd geometry (16-row phases) has no
        switch (sid) {                                            // bias path - as the forward's launch_fwd_ctx
            case 0: return d || ictx ? Kernel::Inv_G8 : Kernel::Inv_G8w;
            case 1: return d ? Kernel::Inv_G16 : Kernel::Inv_G16w;
            case 2: return d ? Kernel::Inv_G32 : Kernel::Inv_G32w;
            case 3: return d ? Kernel::Inv_G64 : Kernel::Inv_G64w2;
            default: return Kernel::None;
        }
    }
    if (pass == Pass::CtxTaped)          // (its backward is cf_flow_step_bwd_taped: direct, one geometry per shape)
        switch (sid) {
            case 0: return Kernel::Step_G8;
            case 1: return Kernel::Step_G16;
            case 2: return Kernel::Step_G32;
            case 3: return Kernel::Step_G64;
            default: return Kernel::None;
        }
    if (pass == Pass::Chain && B > chain_max_batch(sid)) return Kernel::None;
    switch (sid) {
        case 0:                          // mnist's C = 8 level, 16x16 images: k_flow_step_small; Winograd in the evaluation forward only
            if (ctx) return Kernel::Step_G8;
            return (pass != Pass::Taped && !direct) ? Kernel::Small_G8w : Kernel::Small_G8s;
        case 1:                          // 16x16 images: k_flow_step_small, one sample per workgroup, Winograd at every batch size (taped: h1
                                         // reaches the tape from the accumulators there, its LDS plane is in the parity-split order)
            if (direct) return ctx ? Kernel::Step_G16 : Kernel::Small_G16s;
            return Kernel::Small_G16w;
        case 2:
            if (!ctx && B <= kRsMaxB8x8) return Kernel::Rs_G32;
            if (B < kFullMinB8x8) return ctx ? Kernel::Step_G32 : Kernel::Step_G32v2;
            if (direct) return Kernel::Step_G32;
            if (eval && B >= kW24MinB8x8) return Kernel::Step_G32w24;
            return Kernel::Step_G32w;
        case 3:
            if (!ctx && B <= kRs16MaxB4x4) return Kernel::Rs16_G64;      // (taped: one sample per workgroup, as the evaluation forward)
            if (!direct && pass == Pass::Eval && B >= kZeroSkipMinB4x4 && zero_skip_enabled()) return Kernel::Step_G64z24;
            if (!direct && B >= kWinoMinB4x4) return eval ? Kernel::Step_G64w24 : Kernel::Step_G64w2;
            return (!ctx && B < kFullMinB4x4) ? Kernel::Step_G64v2 : Kernel::Step_G64;
    }
    return Kernel::None;
}

// A kernel that a pass's launch list does not hold is a bug in select().
static int not_built(const char* fn, Kernel k) {
    cf_set_error("%s: kernel %d is not built for this pass", fn, (int)k);
    return CF_ERR_UNSUPPORTED;
}
static int unsupported_shape(const char* fn, int C, int H, int W) {
    cf_set_error("%s: shape (%d,%d,%d) unsupported", fn, C, H, W);
    return CF_ERR_UNSUPPORTED;
}
