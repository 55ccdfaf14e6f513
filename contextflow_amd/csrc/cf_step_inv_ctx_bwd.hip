// The vector-Jacobian product of the specialist coupling's inverse (cf_flow_step_inv_ctx): the INV form of k_flow_step_bwd
// (cf_step_bwd.hip) with the per-sample bias in its recompute (IB), in a translation unit of its own for the reason
// cf_step_inv_bwd.hip gives - the kernels of the other units compile to what they were.
#define CF_STEP_BWD_KERNELS_ONLY 1
#include "cf_step_bwd.hip"

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
    CF_REQUIRE(x && gx && ws && wsb && sbias && gz && B >= 0 && (mode == 1 || mode == 2));
    CF_REQUIRE(x_bstride >= (int64_t)C * H * W && x_bstride % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0 &&
               (reinterpret_cast<uintptr_t>(gx) & 15) == 0 && (reinterpret_cast<uintptr_t>(gz) & 15) == 0);
    const float* w = (const float*)ws;
    const float* wb = (const float*)wsb;
    int rc = 0;
#define CF_BWDIC(G)                                                                                                                     \
    rc = mode == 1 ? launch_step_bwd<G, true, true, true, 1>(x, gx, nullptr, w, wb, gz, nullptr, nullptr, nullptr, nullptr, nullptr,   \
                                                            nullptr, nullptr, B, x_bstride, cf_s(stream), sbias)                      \
                   : launch_step_bwd<G, true, true, true, 2>(x, gx, nullptr, w, wb, gz, nullptr, nullptr, nullptr, nullptr, nullptr,   \
                                                            nullptr, nullptr, B, x_bstride, cf_s(stream), sbias)
    switch (shape_id(C, H, W)) {
        case 0: CF_BWDIC(B8); break;
        case 1: CF_BWDIC(B16); break;
        case 2: CF_BWDIC(B32); break;
        case 3: CF_BWDIC(B64); break;
        default: cf_set_error("cf_flow_step_inv_bwd_ctx_data: shape (%d,%d,%d) unsupported", C, H, W); return CF_ERR_UNSUPPORTED;
    }
#undef CF_BWDIC
    if (rc) return rc;
    CF_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
