// Backward of one flow step (Conv1x1 -> ActNorm -> Coupling) for the training step that follows the density
// path (contextflow/experiment_cl.py:130-136 `cost.backward()`), as ONE gfx950 kernel per step.
//
// What the data-gradient chain needs of the forward - y1, the log-scale and the two ReLU masks - comes from the tape the
// training forward wrote (the generalist: cf_flow_step_fwd_taped; no step input, no recompute), or - the specialist coupling
// under contextflow, whose generalist weights are frozen - is recomputed from the step input in LDS with the forward's own
// code.  (A generalist step whose tape was not kept re-runs the taping FORWARD kernel first: layers/autograd.py
// step_backward.)  Then, on the fp32 matrix cores with TRANSPOSED weight fragments:
//     g_h   = [ g_z1 ,  (g_z1 * y1 * e^{ls} + g_ld) * (1 - (ls/2)^2) ]           affine map + log-det
//     g_h2  = (NN.4^T g_h)            * [h2 > 0]
//     g_h1  = (NN.2^T (*) g_h2)       * [h1 > 0]     3x3 transposed conv = adjoint of the reflect-padded gather
//     g_y0  =  NN.0^T g_h1 + g_z0 ;   g_y1 = g_z1 * e^{ls}
//     g_x   = (e^{-logs} Wm)^T g_y
// and writes, next to g_x, the gradient planes the weight gradients contract over (taped form: g_h, g_h2, g_h1, g_y; their
// other operands y0, h1, h2 are the tape's; recompute form: g_h only).  The weight gradients themselves are split-K MFMA
// GEMMs over (sample, pixel): cf_wgrad.hip, called from contextflow_amd/layers/autograd.py.  ReLU masks are 16-bit lane masks
// in registers.
// The adjoint of the reflected gather reads, per tap, ONE source per operand: every LDS plane row carries the fold sums of
// its border rows / columns behind its pixels (PATCH geometries, see patch_build below); 4x4 images keep the class-by-class
// weighted sums (adj_tap<NS>).
#include "cf_step_bwd.h"

// the tape as the backward kernels see it: the aux buffer alone
static StepTape aux_tape(const void* t_aux, int B, int C, int H, int W) {
    constexpr float* none = nullptr;
    return t_aux ? make_tape(none, none, none, const_cast<void*>(t_aux), B, C, H, W) : kNoTape;
}

extern "C" {

int64_t cf_flow_step_bwd_ws_bytes(int C, int H, int W) {
    switch (shape_id(C, H, W)) {
        case 0: return (int64_t)GeoBwd<B8>::WS_FLOATS * 4;
        case 1: return (int64_t)GeoBwd<B16>::WS_FLOATS * 4;
        case 2: return (int64_t)GeoBwd<B32>::WS_FLOATS * 4;
        case 3: return (int64_t)GeoBwd<B64>::WS_FLOATS * 4;
    }
    return 0;
}

int cf_flow_step_bwd_prepare_batch(int n, const float* const* Wm, const float* const* logs, const float* const* w1,
                                   const float* const* w2, const float* const* w3, void* const* wsb, int C, int H, int W,
                                   cf_stream_t stream) {
    CF_REQUIRE(n >= 0 && Wm && logs && w1 && w2 && w3 && wsb);
    const int sid = shape_id(C, H, W);
    if (sid < 0) { cf_set_error("cf_flow_step_bwd_prepare: shape (%d,%d,%d) unsupported", C, H, W); return CF_ERR_UNSUPPORTED; }
    for (int i0 = 0; i0 < n; i0 += kPrepBatchBwd) {
        const int m = n - i0 < kPrepBatchBwd ? n - i0 : kPrepBatchBwd;
        StepPackBwdBatch pb{};
        for (int i = 0; i < m; ++i) {
            const int j = i0 + i;
            CF_REQUIRE(Wm[j] && logs[j] && w1[j] && w2[j] && w3[j] && wsb[j] && (reinterpret_cast<uintptr_t>(wsb[j]) & 15) == 0);
            pb.Wm[i] = Wm[j]; pb.logs[i] = logs[j]; pb.w1[i] = w1[j]; pb.w2[i] = w2[j]; pb.w3[i] = w3[j]; pb.wsb[i] = (float*)wsb[j];
        }
        switch (sid) {
            case 0: launch_prepare_bwd<B8>(pb, m, cf_s(stream)); break;
            case 1: launch_prepare_bwd<B16>(pb, m, cf_s(stream)); break;
            case 2: launch_prepare_bwd<B32>(pb, m, cf_s(stream)); break;
            default: launch_prepare_bwd<B64>(pb, m, cf_s(stream)); break;
        }
        CF_LAUNCH_CHECK();
    }
    return 0;
}

int cf_flow_step_bwd_prepare(const float* Wm, const float* logs, const float* w1, const float* w2, const float* w3,
                             void* wsb, int C, int H, int W, cf_stream_t stream) {
    CF_REQUIRE(Wm && logs && w1 && w2 && w3 && wsb && (reinterpret_cast<uintptr_t>(wsb) & 15) == 0);
    return cf_flow_step_bwd_prepare_batch(1, &Wm, &logs, &w1, &w2, &w3, &wsb, C, H, W, stream);
}

// backward of a step whose forward was cf_flow_step_fwd_taped: the kernel reads ls / y1 / the two ReLU masks from the
// tape's aux buffer - it needs neither the step input nor the forward's packed weights, and runs no recompute.  (The y0 /
// h1 / h2 planes of the tape are operands of cf_wgrad only.)  gx comes out in the (B, C, H, W) layout of the step.
int cf_flow_step_bwd_taped(const float* gz, const float* gld, const void* wsb, const void* t_aux, float* gx, float* s_gh,
                           float* s_gh2, float* s_gh1, float* s_gy, int B, int C, int H, int W, int gx_unsqueezed,
                           cf_stream_t stream) {
    if (B == 0) return 0;
    const StepBwdArgs a{.gz = gz, .gld = gld, .wsb = (const float*)wsb, .gx = gx, .s_gh = s_gh, .s_gh2 = s_gh2, .s_gh1 = s_gh1,
                        .s_gy = s_gy, .B = B, .xbs = (int64_t)C * H * W, .s = cf_s(stream), .tp = aux_tape(t_aux, B, C, H, W),
                        .gx_unsq = gx_unsqueezed != 0};
    if (int rc = check_step_bwd<false, false, false, 0>(__func__, a, C, H, W)) return rc;
    if (int rc = launch_bwd<false>(shape_id(C, H, W), a)) return rc;
    CF_LAUNCH_CHECK();
    return 0;
}

// the data-gradient chain of cf_flow_step_bwd_taped alone (d log p(x) / d x with frozen weights: FlowSequential.score): the same
// kernels with the stores of the four weight-gradient operand planes compiled out, the same dispatch - gx is bitwise equal.
int cf_flow_step_bwd_data(const float* gz, const float* gld, const void* wsb, const void* t_aux, float* gx, int B, int C, int H,
                          int W, int gx_unsqueezed, cf_stream_t stream) {
    if (B == 0) return 0;
    const StepBwdArgs a{.gz = gz, .gld = gld, .wsb = (const float*)wsb, .gx = gx, .B = B, .xbs = (int64_t)C * H * W, .s = cf_s(stream),
                        .tp = aux_tape(t_aux, B, C, H, W), .gx_unsq = gx_unsqueezed != 0};
    if (int rc = check_step_bwd<false, true, false, 0>(__func__, a, C, H, W)) return rc;
    if (int rc = launch_bwd<false, true>(shape_id(C, H, W), a)) return rc;
    CF_LAUNCH_CHECK();
    return 0;
}

// backward of the specialist coupling under contextflow (cf_flow_step_fwd_ctx, mode 1): same kernel, the recompute
// adds the per-sample bias sbias (B, C) to the conditioner output.  d/d sbias[b, c] = sum_p s_gh[b, c, p].
int cf_flow_step_bwd_ctx(const float* x, const float* gz, const float* gld, const void* ws, const void* wsb,
                         const float* sbias, float* gx, float* s_y0, float* s_h1, float* s_h2, float* s_gh, float* s_gh2,
                         float* s_gh1, float* s_gy, int B, int C, int H, int W, int64_t x_bstride, cf_stream_t stream) {
    if (B == 0) return 0;
    const StepBwdArgs a{.x = x, .gz = gz, .gld = gld, .ws = (const float*)ws, .wsb = (const float*)wsb, .gx = gx, .s_y0 = s_y0,
                        .s_h1 = s_h1, .s_h2 = s_h2, .s_gh = s_gh, .s_gh2 = s_gh2, .s_gh1 = s_gh1, .s_gy = s_gy, .B = B,
                        .xbs = x_bstride, .s = cf_s(stream), .bias_or_wsv = sbias};
    if (int rc = check_step_bwd<true, false, false, 0>(__func__, a, C, H, W)) return rc;
    if (int rc = launch_bwd<true>(shape_id(C, H, W), a)) return rc;
    CF_LAUNCH_CHECK();
    return 0;
}

// the data-gradient chain of cf_flow_step_bwd_ctx alone (d log p(x | c) / d x: FlowSequential.score with a context): the same
// kernel and dispatch with the store of the s_gh plane compiled out - gx is bitwise equal.
int cf_flow_step_bwd_ctx_data(const float* x, const float* gz, const float* gld, const void* ws, const void* wsb,
                              const float* sbias, float* gx, int B, int C, int H, int W, int64_t x_bstride, cf_stream_t stream) {
    if (B == 0) return 0;
    const StepBwdArgs a{.x = x, .gz = gz, .gld = gld, .ws = (const float*)ws, .wsb = (const float*)wsb, .gx = gx, .B = B,
                        .xbs = x_bstride, .s = cf_s(stream), .bias_or_wsv = sbias};
    if (int rc = check_step_bwd<true, true, false, 0>(__func__, a, C, H, W)) return rc;
    if (int rc = launch_bwd<true, true>(shape_id(C, H, W), a)) return rc;
    CF_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
