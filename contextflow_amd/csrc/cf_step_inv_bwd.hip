// The vector-Jacobian product of the inverse flow step: the INV form of k_flow_step_bwd (cf_step_bwd.hip), instantiated in a
// translation unit of its own.  Built next to the training and score forms it moves the register allocation of one of THEM
// (k_flow_step_bwd<B64, taped>: 190 -> 189 VGPRs; profiles/decode_grad.md) although no line of their bodies changes - here they
// compile to what they were.
#define CF_STEP_BWD_KERNELS_ONLY 1
#include "cf_step_bwd.hip"

extern "C" {

// the vector-Jacobian product of the INVERSE step (cf_flow_step_inv) at its output: given x, the step input that the inverse
// recovered, and gx = d L / d x, writes gz = d L / d z for the z that cf_flow_step_inv was given.  Data only - no parameter
// gradient is formed.  ws / wsb: the step's forward and transposed tables (cf_flow_step_prepare, cf_flow_step_bwd_prepare);
// wsv: cf_flow_step_inv_bwd_prepare.  One launch, no atomics: two calls give the same bits.
int cf_flow_step_inv_bwd_data(const float* x, const float* gx, const void* ws, const void* wsb, const void* wsv, float* gz,
                              int B, int C, int H, int W, int64_t x_bstride, cf_stream_t stream) {
    if (B == 0) return 0;
    CF_REQUIRE(x && gx && ws && wsb && wsv && gz && B >= 0);
    CF_REQUIRE(x_bstride >= (int64_t)C * H * W && x_bstride % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0 &&
               (reinterpret_cast<uintptr_t>(gx) & 15) == 0 && (reinterpret_cast<uintptr_t>(gz) & 15) == 0 &&
               (reinterpret_cast<uintptr_t>(wsv) & 15) == 0);
    const float* w = (const float*)ws;
    const float* wb = (const float*)wsb;
    int rc = 0;
#define CF_BWDI(G) rc = launch_step_bwd<G, true, true, true>(x, gx, nullptr, w, wb, gz, nullptr, nullptr, nullptr, nullptr, nullptr, \
                                                             nullptr, nullptr, B, x_bstride, cf_s(stream), (const float*)wsv)
    switch (shape_id(C, H, W)) {
        case 0: CF_BWDI(B8); break;
        case 1: CF_BWDI(B16); break;
        case 2: CF_BWDI(B32); break;
        case 3: CF_BWDI(B64); break;
        default: cf_set_error("cf_flow_step_inv_bwd_data: shape (%d,%d,%d) unsupported", C, H, W); return CF_ERR_UNSUPPORTED;
    }
#undef CF_BWDI
    if (rc) return rc;
    CF_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
