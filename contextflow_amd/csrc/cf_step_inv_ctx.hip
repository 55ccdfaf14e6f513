// The specialist coupling backwards in one launch: the CTX form of k_flow_step_inv (cf_step.hip), instantiated in a translation
// unit of its own so that every kernel of cf_step.hip compiles to what it was (cf_step_inv_bwd.hip has the precedent).
#define CF_STEP_KERNELS_ONLY 1
#include "cf_step.hip"

namespace {

template <class G, int CTX>
int launch_step_inv_ctx(const float* z, float* x, const float* ws, const float* sb, int B, int64_t zbs, hipStream_t s) {
    constexpr size_t lds_bytes = (size_t)G::LDS_FLOATS * sizeof(float);
    if (lds_bytes > 64 * 1024) {
        static std::atomic<uint64_t> raised{0};
        if (int rc_ = cf_raise_dynamic_lds((const void*)k_flow_step_inv<G, false, CTX>, 160 * 1024, raised, __func__)) return rc_;
    }
    k_flow_step_inv<G, false, CTX><<<dim3((B + G::SPW - 1) / G::SPW), dim3(256), lds_bytes, s>>>(z, x, ws, sb, B, zbs, 0, nullptr);
    return 0;
}

// One geometry per level, at every batch size: the Winograd geometries Pass::Inverse selects in cf_step.hip, and the direct one
// at C = 8, whose Winograd geometry (16-row phases) has no bias path - as the forward's launch_fwd_ctx.
template <int CTX>
int launch_inv_ctx(int sid, const float* z, float* x, const float* ws, const float* sb, int B, int64_t zbs, hipStream_t s) {
    switch (sid) {
        case 0: return launch_step_inv_ctx<G8, CTX>(z, x, ws, sb, B, zbs, s);
        case 1: return launch_step_inv_ctx<G16w, CTX>(z, x, ws, sb, B, zbs, s);
        case 2: return launch_step_inv_ctx<G32w, CTX>(z, x, ws, sb, B, zbs, s);
        case 3: return launch_step_inv_ctx<G64w2, CTX>(z, x, ws, sb, B, zbs, s);
    }
    return CF_ERR_UNSUPPORTED;
}

}  // namespace

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
    const int sid = shape_id(C, H, W);
    if (sid < 0) {
        cf_set_error("cf_flow_step_inv_ctx: shape (%d,%d,%d) unsupported", C, H, W);
        return CF_ERR_UNSUPPORTED;
    }
    if (int rc = mode == 1 ? launch_inv_ctx<1>(sid, z, x, (const float*)ws, sbias, B, z_bstride, cf_s(stream))
                           : launch_inv_ctx<2>(sid, z, x, (const float*)ws, sbias, B, z_bstride, cf_s(stream)))
        return rc;
    CF_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
