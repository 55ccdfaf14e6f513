// The specialist coupling backwards in one launch: the CTX form of k_flow_step_inv (cf_step_inv.h), instantiated in a translation
// unit of its own so that every kernel that cf_step.hip instantiates compiles to what it was (cf_step_inv_bwd.hip has the precedent).  The
// kernel is select()'s choice for Pass::InverseCtx (cf_step_dispatch.h) and the launch is launch_step_inv with a StepInvArgs:
// this unit holds the launch list of its four instantiations and the entry point.
#include "cf_step_inv.h"
#include "cf_step_dispatch.h"

template <int CTX>
static int launch_inv_ctx(Kernel k, const StepInvArgs& a) {
    switch (k) {
        case Kernel::Inv_G8: return launch_step_inv<G8, false, CTX>(a);
        case Kernel::Inv_G16w: return launch_step_inv<G16w, false, CTX>(a);
        case Kernel::Inv_G32w: return launch_step_inv<G32w, false, CTX>(a);
        case Kernel::Inv_G64w2: return launch_step_inv<G64w2, false, CTX>(a);
        default: return not_built(__func__, k);
    }
}

extern "C" {

// x = [z0 | (z1 - tau) e^{-s}],  [tau | raw] = NN(z0) (+) CN(c),  s = 2 tanh(raw / 2): the inverse of cf_flow_step_fwd_ctx for the
// Coupling layer alone.  ws: the coupling's tables with an identity front (cf_flow_step_prepare); sbias / mode as
// cf_flow_step_fwd_ctx - 1: (B, C) on the conditioner output, 2: (B, 2C) before the first ReLU.  No un-squeeze.  z may be a
// channel / batch slice (z_bstride); alignment as cf_flow_step_inv.  Loads clamp to the last sample, stores cover valid samples.
int cf_flow_step_inv_ctx(const float* z, float* x, const void* ws, const float* sbias, int mode, int B, int C, int H, int W,
                         int64_t z_bstride, cf_stream_t stream) {
    if (B == 0) return 0;                       // empty batch: nothing to do (pointers may be null)
    CF_REQUIRE(z && x && ws && sbias && B >= 0 && (mode == 1 || mode == 2) && z_bstride >= (int64_t)C * H * W && z_bstride % 4 == 0);
    CF_REQUIRE((reinterpret_cast<uintptr_t>(z) & 15) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0);
    const Kernel k = select(Pass::InverseCtx, shape_id(C, H, W), B);
    if (k == Kernel::None) return unsupported_shape(__func__, C, H, W);
    const StepInvArgs a{.z = z, .x = x, .ws = (const float*)ws, .sb = sbias, .B = B, .zbs = z_bstride, .s = cf_s(stream)};
    if (int rc = mode == 1 ? launch_inv_ctx<1>(k, a) : launch_inv_ctx<2>(k, a)) return rc;
    CF_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
