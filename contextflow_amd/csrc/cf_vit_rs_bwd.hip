// Backward of one transformer-coupling flow step (Conv1x1 -> ActNorm -> TransCoupling with its SimpleViT conditioner) as
// ONE kernel + ONE grouped weight-gradient launch: the caller right after the path in the anomaly-detection experiments,
// `cost.backward()` (contextflow/experiment_ad.py:204-213; layers/coupling.py:123-155, layers/simple_vit.py:18-127,
// layers/conv1x1.py:52-57, layers/actnorm.py:53-60).  Round 2 trained these flows layer by layer: ~260 launches per step.
//
// Shape: the row-split workgroup of cf_vit_rs.hip - four waves share 16 token columns (4 samples) and split the output
// rows of every product, planes [feature][16 tokens] in LDS (52.7 KB: three workgroups per CU).  Nothing but the step INPUT is
// kept from the forward:
//   phase A  re-runs the step (the forward kernel's arithmetic) and parks the residual stream at every layer boundary in
//            LDS (the owner wave's tile only: 16 B per lane and layer);
//   phase B  walks back: epilogue (affine map, log-det), final LayerNorm, then per layer - recompute q / k / v, softmax, the
//            attention output, the mid-layer residual, the MLP pre-activation from the parked input; data gradients with
//            TRANSPOSED weight fragments (k_vit_rs_pack_bwd); LayerNorm / softmax / GELU adjoints on the owner's tile, the
//            per-token sums of the LayerNorm adjoints through a two-value exchange between the waves - then the patch
//            embedding and the Conv1x1 + ActNorm product.
// Parameter gradients: every Linear's two operands (its input u and the gradient of its output) leave the kernel as
// token-major planes, coalesced (lane = feature), and ONE launch of the grouped split-K GEMM (cf_linear_wgrad_group,
// cf_vit.hip) contracts all 26 pairs of a step over the tokens; LayerNorm weight / bias gradients are summed over a
// workgroup's 16 tokens in registers and leave as one partial per workgroup (fixed-order reduction afterwards: no float
// atomics, bitwise reproducible).
#include "cf_vit_rs_bwd.h"

extern "C" {

int64_t cf_vit_step_bwd_ws_bytes(int C, int depth) { return C == 26 ? (int64_t)wsb_floats<RS26>(depth) * 4 : 0; }
// floats of the token-major plane buffer / the LayerNorm partial buffer for a batch of B samples
int64_t cf_vit_step_bwd_plane_floats(int B, int C, int depth) {
    if (C != 26) return 0;
    const int64_t Bp = (B + 3) / 4 * 4, R4 = 4 * Bp, P8 = 8 * Bp;
    return 2 * P8 * C + R4 * (RS26::PD + RS26::DIM) + (int64_t)depth * R4 * RB26::TL;
}
int64_t cf_vit_step_bwd_ln_floats(int B, int C, int depth) { return C == 26 ? (int64_t)((B + 3) / 4) * RB26::ln_floats(depth) : 0; }

int cf_vit_step_bwd_prepare_batch(int n, const float* const* Wm, const float* const* logs, const float* const* flat_vit_params,
                                  void* const* wsb, int C, int depth, cf_stream_t stream) {
    CF_REQUIRE(n >= 0 && Wm && logs && flat_vit_params && wsb && depth >= 1 && depth <= kVitMaxDepth);
    if (C != 26) { cf_set_error("cf_vit_step_bwd_prepare_batch: C=%d unsupported", C); return CF_ERR_UNSUPPORTED; }
    for (int i0 = 0; i0 < n; i0 += kVitPrepBatch) {
        const int m = n - i0 < kVitPrepBatch ? n - i0 : kVitPrepBatch;
        VitRsPackBwdBatch pb{};
        for (int i = 0; i < m; ++i) {
            const int j = i0 + i;
            CF_REQUIRE(Wm[j] && logs[j] && flat_vit_params[j] && wsb[j] && (reinterpret_cast<uintptr_t>(wsb[j]) & 15) == 0);
            pb.Wm[i] = Wm[j]; pb.logs[i] = logs[j]; pb.flat[i] = flat_vit_params[j]; pb.wsb[i] = (float*)wsb[j];
        }
        k_vit_rs_pack_bwd<RS26><<<dim3(64, m), dim3(256), 0, cf_s(stream)>>>(pb, depth);
        CF_LAUNCH_CHECK();
    }
    return 0;
}


// xtape (NULL, or the cf_vit_step_tape_floats(B, C, depth) floats a forward with xtape wrote): the six layers are not run a second
// time before the way back.  Same outputs to fp32 rounding (the tape holds the forward's own residual stream, the recompute
// form rebuilds it in the row-split kernel's summation order).
int cf_vit_step_bwd(const float* x, const float* gz, const float* gld, float* gx, const void* ws, const void* wsb, float* planes,
                    float* ln_partials, const float* xtape, int B, int C, int depth, int64_t x_bstride, cf_stream_t stream) {
    if (B == 0) return 0;
    CF_REQUIRE(x && gz && gld && gx && ws && wsb && planes && ln_partials && B > 0 && depth >= 1 && depth <= kVitMaxDepth &&
               x_bstride >= (int64_t)C * 8);
    if (C != 26) { cf_set_error("cf_vit_step_bwd: C=%d unsupported", C); return CF_ERR_UNSUPPORTED; }
    constexpr size_t lds_bytes = (size_t)RB26::LDS_FLOATS * sizeof(float);
    static std::atomic<uint64_t> raised[2];
    const void* kernel = xtape ? (const void*)k_vit_step_bwd_rs<RS26, true> : (const void*)k_vit_step_bwd_rs<RS26>;
    if (int rc_ = cf_raise_dynamic_lds(kernel, 160 * 1024, raised[xtape != nullptr], __func__)) return rc_;
    const int nwg = (B + 3) / 4;
    const dim3 grid((unsigned)nwg), block(256);
    const float *w = (const float*)ws, *wb = (const float*)wsb;
    if (xtape) k_vit_step_bwd_rs<RS26, true><<<grid, block, lds_bytes, cf_s(stream)>>>(x, gz, gld, gx, w, wb, planes, ln_partials, B, nwg * 4,
                                                                                       x_bstride, depth, xtape, vit_tape_tokens(B));
    else k_vit_step_bwd_rs<RS26><<<grid, block, lds_bytes, cf_s(stream)>>>(x, gz, gld, gx, w, wb, planes, ln_partials, B, nwg * 4, x_bstride, depth);
    CF_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
