// The translation unit of the conv flow step's forward and inverse directions: the launch lists - exactly the kernels the library
// builds - the extern "C" entry points and the test hooks.  Host code only; every kernel family is a header with its argument
// record and launch helpers:
//   cf_step_fwd.h       what the forward families share: the design of the fused step, StepArgs, the weight packing, WsChain
//   cf_step_tile.h      k_flow_step and k_flow_step_level (32x32x2 tiles, SPW whole samples per workgroup)
//   cf_step_small.h     k_flow_step_small with its chain and level forms (the 16x16 level)
//   cf_step_rs.h        k_flow_step_rs and k_flow_step_rs16 with their chain forms (small batches at 8x8 and 4x4)
//   cf_step_inv.h       k_flow_step_inv; cf_step_inv_ctx.hip instantiates its CTX form in a unit of its own
//   cf_step_dispatch.h  select(): which kernel runs a step
#include "cf_step_tile.h"
#include "cf_step_small.h"
#include "cf_step_rs.h"
#include "cf_step_inv.h"
#include "cf_step_dispatch.h"

// Multiply-adds per pixel and C^2 of a kernel's step, from its geometry's own traits: the direct form runs C^2 (Conv1x1) + C^2 +
// 36 C^2 + 2 C^2 = 40 C^2, the Winograd form of the 3x3 runs 16 instead of 36 C^2 (F(2x2, 3x3)) or 12 C^2 (F(2x4, 3x3)).
template <class G> constexpr int step_macs_c2hw() { return G::W24 ? 16 : G::WINO ? 20 : 40; }
static int step_macs_c2hw(Kernel k) {
    switch (k) {
        case Kernel::None: return 0;
        case Kernel::Small_G8s: return step_macs_c2hw<G8s>();
        case Kernel::Small_G16s: return step_macs_c2hw<G16s>();
        case Kernel::Small_G8w: case Kernel::Inv_G8w: return step_macs_c2hw<G8w>();
        case Kernel::Small_G16w: case Kernel::Inv_G16w: return step_macs_c2hw<G16w>();
        case Kernel::Step_G8: case Kernel::Inv_G8: return step_macs_c2hw<G8>();
        case Kernel::Step_G16: case Kernel::Inv_G16: return step_macs_c2hw<G16>();
        case Kernel::Step_G32: case Kernel::Rs_G32: case Kernel::Inv_G32: return step_macs_c2hw<G32>();
        case Kernel::Step_G32v2: return step_macs_c2hw<G32v2>();
        case Kernel::Step_G32w: case Kernel::Inv_G32w: return step_macs_c2hw<G32w>();
        case Kernel::Step_G32w24: return step_macs_c2hw<G32w24>();
        case Kernel::Step_G64: case Kernel::Rs16_G64: case Kernel::Inv_G64: return step_macs_c2hw<G64>();
        case Kernel::Step_G64v2: return step_macs_c2hw<G64v2>();
        case Kernel::Step_G64w2: case Kernel::Inv_G64w2: return step_macs_c2hw<G64w2>();
        case Kernel::Step_G64w24: return step_macs_c2hw<G64w24>();
        case Kernel::Step_G64z24: return step_macs_c2hw<G64z24>();      // (the count of the form: the skipped zero products are in it)
    }
    return 0;
}

// Launch lists, one per pass: exactly the template combinations the library builds (a 160 KB k_flow_step instantiation is
// minutes of compile time).  A kernel that a pass does not list is a bug in select() (not_built).
static int launch_fwd(Kernel k, const StepArgs& a) {         // evaluation forward, and the test hook without dumps
    switch (k) {
        case Kernel::Small_G8s: return launch_step_small<G8s>(a);
        case Kernel::Small_G16s: return launch_step_small<G16s>(a);
        case Kernel::Small_G8w: return launch_step_small<G8w>(a);
        case Kernel::Small_G16w: return launch_step_small<G16w>(a);
        case Kernel::Step_G8: return launch_step<G8>(a);
        case Kernel::Step_G16: return launch_step<G16>(a);
        case Kernel::Step_G32: return launch_step<G32>(a);
        case Kernel::Step_G32v2: return launch_step<G32v2>(a);
        case Kernel::Step_G32w: return launch_step<G32w>(a);
        case Kernel::Step_G32w24: return launch_step<G32w24>(a);
        case Kernel::Step_G64: return launch_step<G64>(a);
        case Kernel::Step_G64v2: return launch_step<G64v2>(a);
        case Kernel::Step_G64w2: return launch_step<G64w2>(a);
        case Kernel::Step_G64w24: return launch_step<G64w24>(a);
        case Kernel::Step_G64z24: return launch_step<G64z24>(a);
        case Kernel::Rs_G32: return launch_step_rs<G32, 2>(a);
        case Kernel::Rs16_G64: return launch_step_rs16<G64>(a);
        default: return not_built(__func__, k);
    }
}
static int launch_fwd_dumps(Kernel k, const StepArgs& a) {   // per-phase dumps (tests): the default geometry of each shape, and k_flow_step_small
    switch (k) {
        case Kernel::Small_G8s: return launch_step_small<G8s, true>(a);
        case Kernel::Small_G16s: return launch_step_small<G16s, true>(a);
        case Kernel::Step_G8: return launch_step<G8, 0, false, true>(a);
        case Kernel::Step_G16: return launch_step<G16, 0, false, true>(a);
        case Kernel::Step_G32: return launch_step<G32, 0, false, true>(a);
        case Kernel::Step_G64: return launch_step<G64, 0, false, true>(a);
        default: return not_built(__func__, k);
    }
}
static int launch_fwd_taped(Kernel k, const StepArgs& a) {
    switch (k) {
        case Kernel::Small_G8s: return launch_step_small<G8s, false, true>(a);
        case Kernel::Small_G16s: return launch_step_small<G16s, false, true>(a);
        case Kernel::Small_G16w: return launch_step_small<G16w, false, true>(a);
        case Kernel::Step_G32: return launch_step<G32, 0, true>(a);
        case Kernel::Step_G32v2: return launch_step<G32v2, 0, true>(a);
        case Kernel::Step_G32w: return launch_step<G32w, 0, true>(a);
        case Kernel::Step_G64: return launch_step<G64, 0, true>(a);
        case Kernel::Step_G64v2: return launch_step<G64v2, 0, true>(a);
        case Kernel::Step_G64w2: return launch_step<G64w2, 0, true>(a);
        case Kernel::Rs_G32: return launch_step_rs<G32, 2, true>(a);
        case Kernel::Rs16_G64: return launch_step_rs16<G64, true>(a);
        default: return not_built(__func__, k);
    }
}
template <int CTX>
static int launch_fwd_ctx(Kernel k, const StepArgs& a) {
    switch (k) {
        case Kernel::Small_G16w: return launch_step_small<G16w, false, false, CTX>(a);
        case Kernel::Step_G8: return launch_step<G8, CTX>(a);
        case Kernel::Step_G16: return launch_step<G16, CTX>(a);
        case Kernel::Step_G32: return launch_step<G32, CTX>(a);
        case Kernel::Step_G32w: return launch_step<G32w, CTX>(a);
        case Kernel::Step_G64: return launch_step<G64, CTX>(a);
        case Kernel::Step_G64w2: return launch_step<G64w2, CTX>(a);
        default: return not_built(__func__, k);
    }
}
static int launch_fwd_ctx_taped(Kernel k, const StepArgs& a) {
    switch (k) {
        case Kernel::Step_G8: return launch_step<G8, 2, true>(a);
        case Kernel::Step_G16: return launch_step<G16, 2, true>(a);
        case Kernel::Step_G32: return launch_step<G32, 2, true>(a);
        case Kernel::Step_G64: return launch_step<G64, 2, true>(a);
        default: return not_built(__func__, k);
    }
}
static int launch_fwd_chain(Kernel k, const StepArgs& a, const WsChain& wc, int n) {      // the chained forms of the small-batch kernels
    switch (k) {
        case Kernel::Small_G8w: return launch_step_small_chain<G8w>(a, wc, n);
        case Kernel::Small_G16w: return launch_step_small_chain<G16w>(a, wc, n);
        case Kernel::Rs_G32: return launch_step_rs_chain<G32, 2>(a, wc, n);
        case Kernel::Rs16_G64: return launch_step_rs16_chain<G64>(a, wc, n);
        default: return not_built(__func__, k);
    }
}
static int launch_fwd_level(Kernel k, const StepArgs& a, const WsChain& wc, int n) {      // the level forms of the saturating-batch kernels
    switch (k) {
        case Kernel::Small_G8w: return launch_step_small_level<G8w>(a, wc, n);
        case Kernel::Small_G16w: return launch_step_small_level<G16w>(a, wc, n);
        case Kernel::Step_G32w24: return launch_step_level<G32w24>(a, wc, n);
        case Kernel::Step_G64w24: return launch_step_level<G64w24>(a, wc, n);
        default: return not_built(__func__, k);
    }
}
// smallest batch at which the evaluation forward of a shape is its saturating-batch kernel (0: the shape has no level form)
static int level_min_batch(int sid) {
    if (direct_conv_only()) return 0;
    switch (sid) {
        case 0: case 1: return kChainMaxB16x16 + 1;
        case 2: return kW24MinB8x8;
        case 3: return kWinoMinB4x4;
    }
    return 0;
}
// the inverse step; LD: with the log-det of the step next to x (cf_flow_step_inv_ld) - the dispatch's choice, its flagged twin
template <bool LD>
static int launch_inv(Kernel k, const StepInvArgs& a) {
    switch (k) {
        case Kernel::Inv_G8: return launch_step_inv<G8, LD>(a);
        case Kernel::Inv_G8w: return launch_step_inv<G8w, LD>(a);
        case Kernel::Inv_G16: return launch_step_inv<G16, LD>(a);
        case Kernel::Inv_G16w: return launch_step_inv<G16w, LD>(a);
        case Kernel::Inv_G32: return launch_step_inv<G32, LD>(a);
        case Kernel::Inv_G32w: return launch_step_inv<G32w, LD>(a);
        case Kernel::Inv_G64: return launch_step_inv<G64, LD>(a);
        case Kernel::Inv_G64w2: return launch_step_inv<G64w2, LD>(a);
        default: return not_built(__func__, k);
    }
}
// (instantiated here, the plain form first: the sixteen kernels keep their place in the code object, whose assembly is what it was)
template int launch_inv<false>(Kernel, const StepInvArgs&);
template int launch_inv<true>(Kernel, const StepInvArgs&);

// test hook: (shape, variant = flags bits 16..19) -> kernel.  0: the default geometry of the shape in k_flow_step (the only one
// with per-phase dumps besides 3), 2: half the samples per workgroup, 3: k_flow_step_small in the direct form, 4: Winograd
// F(2x2, 3x3), 5: ... row-split at 128 pixels per workgroup, 6: Winograd F(2x4, 3x3) at 8x8 and 4x4, 7 (4x4): ... with 16 samples
// on 8 waves, skipping the zero products.  (1 was an operand-pipeline alternate of each shape, 6 at 16x16 and 7 at 16x16 two forms
// on the 16-bit matrix cores: gone with their geometries.)
template <class G>
static int lane_table_copy(int* out, int cap) {      // host copy of kLaneTab<G> (cf_lane_table_debug): same constexpr initialiser
    static const LaneTab<G> tab = make_lane_tab<G>();
    constexpr int n = (int)(sizeof(LaneEntry<G>) / sizeof(int));
    static_assert(sizeof(tab) == 256 * n * sizeof(int), "an entry is n ints, no padding");
    const int* src = reinterpret_cast<const int*>(&tab);
    for (int i = 0; out && i < cap && i < 256 * n; ++i) out[i] = src[i];
    return n;
}
constexpr int kDebugVariants = 8;
constexpr Kernel kDebugKernel[4][kDebugVariants] = {
    {Kernel::Step_G8, Kernel::None, Kernel::None, Kernel::Small_G8s, Kernel::Small_G8w, Kernel::None, Kernel::None, Kernel::None},
    {Kernel::Step_G16, Kernel::None, Kernel::None, Kernel::Small_G16s, Kernel::Small_G16w, Kernel::None, Kernel::None, Kernel::None},
    {Kernel::Step_G32, Kernel::None, Kernel::Step_G32v2, Kernel::None, Kernel::Step_G32w, Kernel::None, Kernel::Step_G32w24, Kernel::None},
    {Kernel::Step_G64, Kernel::None, Kernel::Step_G64v2, Kernel::None, Kernel::None, Kernel::Step_G64w2, Kernel::Step_G64w24, Kernel::Step_G64z24},
};

extern "C" {

int cf_flow_step_supported(int C, int H, int W, int kh, int kw) {
    return (kh == 3 && kw == 3 && shape_id(C, H, W) >= 0) ? 1 : 0;
}

int64_t cf_flow_step_ws_bytes(int C, int H, int W) {
    switch (shape_id(C, H, W)) {
        case 0: return (int64_t)G8::WS_FLOATS * 4;
        case 1: return (int64_t)G16::WS_FLOATS * 4;
        case 2: return (int64_t)G32::WS_FLOATS * 4;
        case 3: return (int64_t)G64::WS_FLOATS * 4;
    }
    return 0;
}

int cf_flow_step_prepare_batch(int n, const float* const* Wm, const float* const* t, const float* const* logs, const float* const* w1,
                               const float* const* b1, const float* const* w2, const float* const* b2, const float* const* w3,
                               const float* const* b3, void* const* ws, float* const* winv, int C, int H, int W, cf_stream_t stream) {
    CF_REQUIRE(n >= 0 && Wm && t && logs && w1 && b1 && w2 && b2 && w3 && b3 && ws);
    const int sid = shape_id(C, H, W);
    if (sid < 0) { cf_set_error("cf_flow_step_prepare: shape (%d,%d,%d) unsupported", C, H, W); return CF_ERR_UNSUPPORTED; }
    for (int i0 = 0; i0 < n; i0 += kPrepBatch) {
        const int m = n - i0 < kPrepBatch ? n - i0 : kPrepBatch;
        StepPackBatch pb{};
        // (the training tables too: they are bitwise those of the evaluation forward - test_prepare_train_equals_prepare_plus_inverse)
        pb.w24 = !direct_conv_only();
        for (int i = 0; i < m; ++i) {
            const int j = i0 + i;
            CF_REQUIRE(Wm[j] && t[j] && logs[j] && w1[j] && b1[j] && w2[j] && b2[j] && w3[j] && b3[j] && ws[j] &&
                       (reinterpret_cast<uintptr_t>(ws[j]) & 15) == 0 && (!winv || winv[j]));
            pb.Wm[i] = Wm[j]; pb.t[i] = t[j]; pb.logs[i] = logs[j]; pb.w1[i] = w1[j]; pb.b1[i] = b1[j]; pb.w2[i] = w2[j]; pb.b2[i] = b2[j];
            pb.w3[i] = w3[j]; pb.b3[i] = b3[j]; pb.ws[i] = (float*)ws[j];
        }
        int rc = 0;
        switch (sid) {
            case 0: rc = launch_prepare<G8>(pb, m, winv ? winv + i0 : nullptr, cf_s(stream)); break;
            case 1: rc = launch_prepare<G16>(pb, m, winv ? winv + i0 : nullptr, cf_s(stream)); break;
            case 2: rc = launch_prepare<G32>(pb, m, winv ? winv + i0 : nullptr, cf_s(stream)); break;
            default: rc = launch_prepare<G64>(pb, m, winv ? winv + i0 : nullptr, cf_s(stream)); break;
        }
        if (rc) return rc;
        CF_LAUNCH_CHECK();
    }
    return 0;
}

int cf_flow_step_prepare(const float* Wm, const float* t, const float* logs, const float* w1, const float* b1,
                         const float* w2, const float* b2, const float* w3, const float* b3, void* ws, int C, int H, int W,
                         cf_stream_t stream) {
    CF_REQUIRE(Wm && t && logs && w1 && b1 && w2 && b2 && w3 && b3 && ws && (reinterpret_cast<uintptr_t>(ws) & 15) == 0);
    return cf_flow_step_prepare_batch(1, &Wm, &t, &logs, &w1, &b1, &w2, &b2, &w3, &b3, &ws, nullptr, C, H, W, stream);
}

int cf_flow_step_prepare_train(const float* Wm, const float* t, const float* logs, const float* w1, const float* b1,
                               const float* w2, const float* b2, const float* w3, const float* b3, void* ws, float* winv,
                               int C, int H, int W, cf_stream_t stream) {
    CF_REQUIRE(Wm && t && logs && w1 && b1 && w2 && b2 && w3 && b3 && ws && winv && (reinterpret_cast<uintptr_t>(ws) & 15) == 0);
    return cf_flow_step_prepare_batch(1, &Wm, &t, &logs, &w1, &b1, &w2, &b2, &w3, &b3, &ws, &winv, C, H, W, stream);
}

int64_t cf_flow_step_inv_ws_bytes(int C, int H, int W) {
    switch (shape_id(C, H, W)) {
        case 0: return (int64_t)(GeoInv<G8>::WS_FLOATS + 4) * 4;
        case 1: return (int64_t)(GeoInv<G16>::WS_FLOATS + 4) * 4;
        case 2: return (int64_t)(GeoInv<G32>::WS_FLOATS + 4) * 4;
        case 3: return (int64_t)(GeoInv<G64>::WS_FLOATS + 4) * 4;
    }
    return 0;
}

int cf_flow_step_inv_prepare(const float* Wm, const float* t, const float* logs, void* wsi, int C, int H, int W,
                             cf_stream_t stream) {
    CF_REQUIRE(Wm && t && logs && wsi && (reinterpret_cast<uintptr_t>(wsi) & 15) == 0);
    int rc;
    float* w = (float*)wsi;
    switch (shape_id(C, H, W)) {
        case 0: rc = launch_prepare_inv<G8>(Wm, t, logs, w, cf_s(stream)); break;
        case 1: rc = launch_prepare_inv<G16>(Wm, t, logs, w, cf_s(stream)); break;
        case 2: rc = launch_prepare_inv<G32>(Wm, t, logs, w, cf_s(stream)); break;
        case 3: rc = launch_prepare_inv<G64>(Wm, t, logs, w, cf_s(stream)); break;
        default: cf_set_error("cf_flow_step_inv_prepare: shape (%d,%d,%d) unsupported", C, H, W); return CF_ERR_UNSUPPORTED;
    }
    if (rc) return rc;
    CF_LAUNCH_CHECK();
    return 0;
}

int64_t cf_flow_step_inv_bwd_ws_bytes(int C, int H, int W) {
    switch (shape_id(C, H, W)) {
        case 0: return (int64_t)G8::NG0 * G8::RT03 * 256 * 4;
        case 1: return (int64_t)G16::NG0 * G16::RT03 * 256 * 4;
        case 2: return (int64_t)G32::NG0 * G32::RT03 * 256 * 4;
        case 3: return (int64_t)G64::NG0 * G64::RT03 * 256 * 4;
    }
    return 0;
}

int cf_flow_step_inv_bwd_prepare(const void* wsi, const float* logs, void* wsv, int C, int H, int W, cf_stream_t stream) {
    CF_REQUIRE(wsi && logs && wsv && (reinterpret_cast<uintptr_t>(wsv) & 15) == 0);
    const float* wi = (const float*)wsi;
    float* wv = (float*)wsv;
    switch (shape_id(C, H, W)) {
        case 0: k_step_pack_inv_bwd<G8><<<dim3(4), dim3(256), 0, cf_s(stream)>>>(wi, logs, wv); break;
        case 1: k_step_pack_inv_bwd<G16><<<dim3(4), dim3(256), 0, cf_s(stream)>>>(wi, logs, wv); break;
        case 2: k_step_pack_inv_bwd<G32><<<dim3(4), dim3(256), 0, cf_s(stream)>>>(wi, logs, wv); break;
        case 3: k_step_pack_inv_bwd<G64><<<dim3(4), dim3(256), 0, cf_s(stream)>>>(wi, logs, wv); break;
        default: cf_set_error("cf_flow_step_inv_bwd_prepare: shape (%d,%d,%d) unsupported", C, H, W); return CF_ERR_UNSUPPORTED;
    }
    CF_LAUNCH_CHECK();
    return 0;
}

int cf_flow_step_inv(const float* z, float* x, const void* ws, const void* wsi, int B, int C, int H, int W,
                     int64_t z_bstride, int x_unsqueezed, cf_stream_t stream) {
    if (B == 0) return 0;                       // empty batch: nothing to do (pointers may be null)
    CF_REQUIRE(z && x && ws && wsi && B >= 0 && z_bstride >= (int64_t)C * H * W && z_bstride % 4 == 0);
    CF_REQUIRE((reinterpret_cast<uintptr_t>(z) & 15) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0);
    const Kernel k = select(Pass::Inverse, shape_id(C, H, W), B);
    if (k == Kernel::None) return unsupported_shape(__func__, C, H, W);
    if (int rc = launch_inv<false>(k, StepInvArgs{.z = z, .x = x, .ws = (const float*)ws, .wsi = (const float*)wsi, .B = B, .zbs = z_bstride,
                                                  .x_unsq = x_unsqueezed, .s = cf_s(stream)}))
        return rc;
    CF_LAUNCH_CHECK();
    return 0;
}

int cf_flow_step_inv_ld(const float* z, float* x, float* ld_acc, const void* ws, const void* wsi, int B, int C, int H, int W,
                        int64_t z_bstride, int x_unsqueezed, cf_stream_t stream) {
    if (B == 0) return 0;                       // empty batch: nothing to do (pointers may be null)
    CF_REQUIRE(z && x && ld_acc && ws && wsi && B >= 0 && z_bstride >= (int64_t)C * H * W && z_bstride % 4 == 0);
    CF_REQUIRE((reinterpret_cast<uintptr_t>(z) & 15) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0);
    const Kernel k = select(Pass::Inverse, shape_id(C, H, W), B);
    if (k == Kernel::None) return unsupported_shape(__func__, C, H, W);
    if (int rc = launch_inv<true>(k, StepInvArgs{.z = z, .x = x, .ld = ld_acc, .ws = (const float*)ws, .wsi = (const float*)wsi, .B = B,
                                                 .zbs = z_bstride, .x_unsq = x_unsqueezed, .s = cf_s(stream)}))
        return rc;
    CF_LAUNCH_CHECK();
    return 0;
}

// test hook (not part of the public header): the step in the kernel of kDebugKernel, and per-phase dumps
int cf_flow_step_fwd_debug(const float* x, float* z, float* ldj_acc, const void* ws, int B, int C, int H, int W,
                           int64_t x_bstride, int in_squeeze, float* dbg, int flags, cf_stream_t stream) {
    if (B == 0) return 0;                       // empty batch: nothing to do (pointers may be null)
    CF_REQUIRE(x && z && ldj_acc && ws && B >= 0 && x_bstride >= (int64_t)C * H * W);
    CF_REQUIRE((reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(z) & 15) == 0 && x_bstride % 4 == 0);
    const int sid = shape_id(C, H, W), variant = (flags >> 16) & 15;
    const Kernel k = (sid >= 0 && variant < kDebugVariants) ? kDebugKernel[sid][variant] : Kernel::None;
    if (k == Kernel::None) {
        cf_set_error("cf_flow_step_fwd: shape (%d,%d,%d) variant %d unsupported", C, H, W, variant);
        return CF_ERR_UNSUPPORTED;
    }
    StepArgs a{x, z, ldj_acc, (const float*)ws, B, x_bstride, in_squeeze != 0, cf_s(stream)};
    a.dbg = dbg;
    if (int rc = dbg ? launch_fwd_dumps(k, a) : launch_fwd(k, a)) return rc;
    CF_LAUNCH_CHECK();
    return 0;
}
// test hook (not part of the public header; host only): the smallest batch at which cf_flow_step_fwd runs this shape's step in the
// zero-skipping F(2x4) kernel (G64z24) - 0 where it never does (other shapes, switched off, CONTEXTFLOW_DIRECT_CONV=1); and the
// A/B switch of that dispatch (on by default; returns what it was).  The debug variants are not affected.
int cf_flow_step_zero_skip_min_batch(int C, int H, int W) {
    return select(Pass::Eval, shape_id(C, H, W), kZeroSkipMinB4x4) == Kernel::Step_G64z24 ? kZeroSkipMinB4x4 : 0;
}
int cf_flow_step_zero_skip_enable(int on) { return g_zero_skip.exchange(on != 0) ? 1 : 0; }
// test hook (not part of the public header; host only): the per-lane address table the saturating-batch kernels of a shape read
// (kLaneTab, cf_step_common.h) as 256 x n ints, thread-major.  Returns n, the ints per thread - 0 for a shape whose kernels derive
// their addresses - and copies min(cap, 256 n) ints to `out`.
int cf_lane_table_debug(int C, int H, int W, int* out, int cap) {
    switch (shape_id(C, H, W)) {
        case 1: static_assert(kLaneTabW22<G16w>, "16x16, C = 16: F(2x2) table"); return lane_table_copy<G16w>(out, cap);
        case 2: static_assert(kLaneTabW24<G32w24>, "8x8: F(2x4) table"); return lane_table_copy<G32w24>(out, cap);    }
    return 0;
}
// n <= 4 consecutive flow steps of one shape in ONE launch, for the batch sizes at which a step is one of the small-batch
// kernels anyway (cf_flow_step_chain_max_batch: 16x16 images up to 1 024 samples, 8x8 up to 512, 4x4 up to 1 024); ws: HOST array
// of the n packed tables; in_squeeze applies to the first step.  z receives the output of the LAST step (the intermediate
// activations live in z too: the steps after the first run in place).  Same numbers as n calls of cf_flow_step_fwd, bit for bit.
int cf_flow_step_chain_max_batch(int C, int H, int W) { return chain_max_batch(shape_id(C, H, W)); }

int cf_flow_step_fwd_chain(const float* x, float* z, float* ldj_acc, const void* const* ws, int n, int B, int C, int H, int W,
                           int64_t x_bstride, int in_squeeze, cf_stream_t stream) {
    if (B == 0 || n == 0) return 0;
    CF_REQUIRE(x && z && ldj_acc && ws && n >= 1 && n <= kChain && B > 0 && x_bstride >= (int64_t)C * H * W);
    CF_REQUIRE((reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(z) & 15) == 0 && x_bstride % 4 == 0);
    const Kernel k = select(Pass::Chain, shape_id(C, H, W), B);
    if (k == Kernel::None) {
        cf_set_error("cf_flow_step_fwd_chain: shape (%d,%d,%d) at a batch of %d is not a chained case", C, H, W, B);
        return CF_ERR_UNSUPPORTED;
    }
    WsChain wc{};
    for (int i = 0; i < n; ++i) { CF_REQUIRE(ws[i]); wc.ws[i] = (const float*)ws[i]; }
    if (int rc = launch_fwd_chain(k, StepArgs{x, z, ldj_acc, nullptr, B, x_bstride, in_squeeze != 0, cf_s(stream)}, wc, n)) return rc;
    CF_LAUNCH_CHECK();
    return 0;
}

// Level form for saturating batches: the n <= 4 consecutive steps of one shape in ONE launch with z in LDS from step to step (x is
// read once, z written once).  form 0: the level form of the kernel cf_flow_step_fwd runs at this batch - from
// cf_flow_step_level_min_batch samples on; below, CF_ERR_UNSUPPORTED and nothing is launched.  form 1 (tests): the saturating-batch
// geometry at any B >= 1.  Same numbers as n calls of that kernel, bit for bit.
int cf_flow_step_level_min_batch(int C, int H, int W) { return level_min_batch(shape_id(C, H, W)); }

int cf_flow_step_fwd_level(const float* x, float* z, float* ldj_acc, const void* const* ws, int n, int B, int C, int H, int W,
                           int64_t x_bstride, int in_squeeze, int form, cf_stream_t stream) {
    if (B == 0 || n == 0) return 0;
    CF_REQUIRE(x && z && x != z && ldj_acc && ws && n >= 1 && n <= kChain && B > 0 && x_bstride >= (int64_t)C * H * W && (form == 0 || form == 1));
    CF_REQUIRE((reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(z) & 15) == 0 && x_bstride % 4 == 0);
    const int sid = shape_id(C, H, W), minb = level_min_batch(sid);
    if (sid < 0) return unsupported_shape(__func__, C, H, W);
    if (minb == 0 || (form == 0 && B < minb)) {
        cf_set_error("cf_flow_step_fwd_level: shape (%d,%d,%d) at a batch of %d is not a level case", C, H, W, B);
        return CF_ERR_UNSUPPORTED;
    }
    const Kernel k = select(Pass::Level, sid, form == 1 && B < minb ? minb : B);
    WsChain wc{};
    for (int i = 0; i < n; ++i) { CF_REQUIRE(ws[i]); wc.ws[i] = (const float*)ws[i]; }
    if (int rc = launch_fwd_level(k, StepArgs{x, z, ldj_acc, nullptr, B, x_bstride, in_squeeze != 0, cf_s(stream)}, wc, n)) return rc;
    CF_LAUNCH_CHECK();
    return 0;
}

int cf_flow_step_fwd(const float* x, float* z, float* ldj_acc, const void* ws, int B, int C, int H, int W,
                     int64_t x_bstride, int in_squeeze, cf_stream_t stream) {
    if (B == 0) return 0;                       // empty batch: nothing to do (pointers may be null)
    CF_REQUIRE(x && z && ldj_acc && ws && B >= 0 && x_bstride >= (int64_t)C * H * W);
    CF_REQUIRE((reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(z) & 15) == 0 && x_bstride % 4 == 0);
    const Kernel k = select(Pass::Eval, shape_id(C, H, W), B);
    if (k == Kernel::None) return unsupported_shape(__func__, C, H, W);
    if (int rc = launch_fwd(k, StepArgs{x, z, ldj_acc, (const float*)ws, B, x_bstride, in_squeeze != 0, cf_s(stream)})) return rc;
    CF_LAUNCH_CHECK();
    return 0;
}

// Multiply-adds per sample the matrix pipe EXECUTES for one step at this batch size (bench.py's executed-flop roofline):
// pass 0 = cf_flow_step_fwd, 1 = cf_flow_step_fwd_taped, 2 = cf_flow_step_bwd_taped (direct transposed 3x3), 3 = cf_flow_step_inv
// (the forward's conditioner + W^-1 instead of W: the same count; Winograd form at every level).  Passes 0, 1 and 3 are the
// count of the kernel select() names for these arguments - the one the entry point launches.
int64_t cf_flow_step_macs(int B, int C, int H, int W, int pass) {
    const int sid = shape_id(C, H, W);
    if (sid < 0 || pass < 0 || pass > 3) return 0;
    const int per = pass == 2 ? step_macs_c2hw<G64>()         // (the backward's geometries are direct ones: any of them)
                              : step_macs_c2hw(select(pass == 0 ? Pass::Eval : pass == 1 ? Pass::Taped : Pass::Inverse, sid, B));
    return (int64_t)per * C * C * H * W;
}

// training forward: the same step, and the conditioner's intermediate planes y0 (B, C/2, H, W), h1, h2 (B, 2C, H, W;
// post-ReLU) go to the caller's tape.  cf_flow_step_bwd_taped consumes them: it skips the recompute of the two big
// contractions and uses the planes directly as the operands of the weight-gradient GEMMs.
int64_t cf_flow_step_tape_aux_bytes(int B, int C, int H, int W) {
    return shape_id(C, H, W) < 0 ? 0 : tape_aux_bytes(B, C, H, W);
}

// (small batches - the reference trains with 256 samples - take the small-batch kernels of the evaluation forward)
int cf_flow_step_fwd_taped(const float* x, float* z, float* ldj_acc, const void* ws, float* t_y0, float* t_h1, float* t_h2,
                           void* t_aux, int B, int C, int H, int W, int64_t x_bstride, int in_squeeze, cf_stream_t stream) {
    if (B == 0) return 0;
    CF_REQUIRE(x && z && ldj_acc && ws && t_y0 && t_h1 && t_h2 && t_aux && x_bstride >= (int64_t)C * H * W && x_bstride % 4 == 0);
    CF_REQUIRE((reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(z) & 15) == 0 &&
               (reinterpret_cast<uintptr_t>(t_y0) & 15) == 0 && (reinterpret_cast<uintptr_t>(t_h1) & 15) == 0 &&
               (reinterpret_cast<uintptr_t>(t_h2) & 15) == 0 && (reinterpret_cast<uintptr_t>(t_aux) & 15) == 0);
    const Kernel k = select(Pass::Taped, shape_id(C, H, W), B);
    if (k == Kernel::None) return unsupported_shape(__func__, C, H, W);
    StepArgs a{x, z, ldj_acc, (const float*)ws, B, x_bstride, in_squeeze != 0, cf_s(stream)};
    a.tp = make_tape(t_y0, t_h1, t_h2, t_aux, B, C, H, W);
    if (int rc = launch_fwd_taped(k, a)) return rc;
    CF_LAUNCH_CHECK();
    return 0;
}

// specialist coupling (coupling.py:39-47): the same fused step with a per-sample bias from the CN net.
// mode 1: sbias (B, C) added to the conditioner OUTPUT (contextflow); mode 2: sbias (B, 2C) added before the first ReLU
// (CN(c) concatenated to the conditioner input).  The caller packs `ws` with cf_flow_step_prepare; with an identity
// matrix / zero ActNorm there, the kernel is the Coupling layer alone (per-sample Conv1x1 / ActNorm run before it).
// mode | 4: the direct form of the 3x3 whatever the batch size (Pass::CtxDirect).
int cf_flow_step_fwd_ctx(const float* x, float* z, float* ldj_acc, const void* ws, const float* sbias, int mode, int B, int C,
                         int H, int W, int64_t x_bstride, cf_stream_t stream) {
    if (B == 0) return 0;
    const Pass pass = (mode & 4) ? Pass::CtxDirect : Pass::Ctx;
    mode &= 3;
    CF_REQUIRE(x && z && ldj_acc && ws && sbias && (mode == 1 || mode == 2) && B >= 0 && x_bstride >= (int64_t)C * H * W);
    CF_REQUIRE((reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(z) & 15) == 0 && x_bstride % 4 == 0);
    const Kernel k = select(pass, shape_id(C, H, W), B);
    if (k == Kernel::None) return unsupported_shape(__func__, C, H, W);
    StepArgs a{x, z, ldj_acc, (const float*)ws, B, x_bstride, false, cf_s(stream)};
    a.sb = sbias;
    if (int rc = mode == 1 ? launch_fwd_ctx<1>(k, a) : launch_fwd_ctx<2>(k, a)) return rc;
    CF_LAUNCH_CHECK();
    return 0;
}

// training forward of the specialist coupling WITHOUT contextflow (mode 2: CN(c) enters before the first ReLU and every
// parameter trains): cf_flow_step_fwd_ctx that also writes the tape planes of cf_flow_step_fwd_taped.  The per-sample
// bias only shapes h1, which the backward loads - cf_flow_step_bwd_taped needs no context argument.
int cf_flow_step_fwd_ctx_taped(const float* x, float* z, float* ldj_acc, const void* ws, const float* sbias, float* t_y0,
                               float* t_h1, float* t_h2, void* t_aux, int B, int C, int H, int W, int64_t x_bstride,
                               cf_stream_t stream) {
    if (B == 0) return 0;
    CF_REQUIRE(x && z && ldj_acc && ws && sbias && t_y0 && t_h1 && t_h2 && t_aux && x_bstride >= (int64_t)C * H * W && x_bstride % 4 == 0);
    CF_REQUIRE((reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(z) & 15) == 0 &&
               (reinterpret_cast<uintptr_t>(t_y0) & 15) == 0 && (reinterpret_cast<uintptr_t>(t_h1) & 15) == 0 &&
               (reinterpret_cast<uintptr_t>(t_h2) & 15) == 0 && (reinterpret_cast<uintptr_t>(t_aux) & 15) == 0);
    const Kernel k = select(Pass::CtxTaped, shape_id(C, H, W), B);
    if (k == Kernel::None) return unsupported_shape(__func__, C, H, W);
    StepArgs a{x, z, ldj_acc, (const float*)ws, B, x_bstride, false, cf_s(stream)};
    a.sb = sbias;
    a.tp = make_tape(t_y0, t_h1, t_h2, t_aux, B, C, H, W);
    if (int rc = launch_fwd_ctx_taped(k, a)) return rc;
    CF_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
