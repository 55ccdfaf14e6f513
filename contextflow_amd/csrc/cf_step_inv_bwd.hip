// The vector-Jacobian product of the inverse flow step: the INV form of k_flow_step_bwd (cf_step_bwd.h), instantiated in a
// translation unit of its own.  Built next to the training and score forms it moves the register allocation of one of THEM
// (k_flow_step_bwd<B64, taped>: 190 -> 189 VGPRs; profiles/decode_grad.md) although no line of their bodies changes - here they
// compile to what they were.  The argument record, the check and the dispatch (StepBwdArgs, check_step_bwd, launch_bwd) are the
// family's, from that header: this unit holds the entry point alone.
#include "cf_step_bwd.h"

extern "C" {

// the vector-Jacobian product of the INVERSE step (cf_flow_step_inv) at its output: given x, the step input that the inverse
// recovered, and gx = d L / d x, writes gz = d L / d z for the z that cf_flow_step_inv was given.  Data only - no parameter
// gradient is formed.  ws / wsb: the step's forward and transposed tables (cf_flow_step_prepare, cf_flow_step_bwd_prepare);
// wsv: cf_flow_step_inv_bwd_prepare.  One launch, no atomics: two calls give the same bits.
int cf_flow_step_inv_bwd_data(const float* x, const float* gx, const void* ws, const void* wsb, const void* wsv, float* gz,
                              int B, int C, int H, int W, int64_t x_bstride, cf_stream_t stream) {
    if (B == 0) return 0;
    CF_REQUIRE(B >= 0);
    // the kernel's upstream / result slots: it is given d/dx and writes d/dz
    const StepBwdArgs a{.x = x, .gz = gx, .ws = (const float*)ws, .wsb = (const float*)wsb, .gx = gz, .B = B, .xbs = x_bstride,
                        .s = cf_s(stream), .bias_or_wsv = wsv};
    if (int rc = check_step_bwd<true, true, true, 0>(__func__, a, C, H, W)) return rc;
    if (int rc = launch_bwd<true, true, true>(shape_id(C, H, W), a)) return rc;
    CF_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
