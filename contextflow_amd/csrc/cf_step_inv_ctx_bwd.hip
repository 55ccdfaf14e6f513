// The vector-Jacobian product of the specialist coupling's inverse (cf_flow_step_inv_ctx): the INV form of k_flow_step_bwd
// (cf_step_bwd.h) with the per-sample bias in its recompute (IB), in a translation unit of its own for the reason
// cf_step_inv_bwd.hip gives - the kernels of the other units compile to what they were.  Record, check and dispatch are the
// family's (StepBwdArgs, check_step_bwd, launch_bwd): this unit holds the entry point alone.
#include "cf_step_bwd.h"

namespace {
// the eight instantiations of this unit, in the order their kernels have in its code object (the two modes of a geometry side by side)
template int launch_step_bwd<B8, true, true, true, 1>(const StepBwdArgs&);
template int launch_step_bwd<B8, true, true, true, 2>(const StepBwdArgs&);
template int launch_step_bwd<B16, true, true, true, 1>(const StepBwdArgs&);
template int launch_step_bwd<B16, true, true, true, 2>(const StepBwdArgs&);
template int launch_step_bwd<B32, true, true, true, 1>(const StepBwdArgs&);
template int launch_step_bwd<B32, true, true, true, 2>(const StepBwdArgs&);
template int launch_step_bwd<B64, true, true, true, 1>(const StepBwdArgs&);
template int launch_step_bwd<B64, true, true, true, 2>(const StepBwdArgs&);
}  // namespace

extern "C" {

// Given x, the coupling input that cf_flow_step_inv_ctx recovered, and gx = d L / d x, writes gz = d L / d z:
//     g_z1 = g_x1 e^{-s},   g_h = [ -g_z1 | -g_x1 x1 (1 - tanh^2(raw / 2)) ],   g_z0 = g_x0 + (d NN / d z0)^T g_h
// with [tau | raw] = NN(x0) (+) CN(c) recomputed from x.  ws: the coupling's tables with an identity front
// (cf_flow_step_prepare); wsb: cf_flow_step_bwd_prepare with an identity matrix and zero logs; sbias / mode: those of
// cf_flow_step_fwd_ctx (1: (B, C) on the conditioner output, 2: (B, 2C) before the first ReLU).  Data only: no gradient with
// respect to a parameter or to sbias.  One launch, no atomics: two calls give the same bits.
int cf_flow_step_inv_bwd_ctx_data(const float* x, const float* gx, const void* ws, const void* wsb, const float* sbias,
                                  int mode, float* gz, int B, int C, int H, int W, int64_t x_bstride, cf_stream_t stream) {
    if (B == 0) return 0;
    CF_REQUIRE(B >= 0 && (mode == 1 || mode == 2));
    // the kernel's upstream / result slots: it is given d/dx and writes d/dz
    const StepBwdArgs a{.x = x, .gz = gx, .ws = (const float*)ws, .wsb = (const float*)wsb, .gx = gz, .B = B, .xbs = x_bstride,
                        .s = cf_s(stream), .bias_or_wsv = sbias};
    if (int rc = check_step_bwd<true, true, true, 1>(__func__, a, C, H, W)) return rc;          // (the two modes require the same)
    const int sid = shape_id(C, H, W);
    if (int rc = mode == 1 ? launch_bwd<true, true, true, 1>(sid, a) : launch_bwd<true, true, true, 2>(sid, a)) return rc;
    CF_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
