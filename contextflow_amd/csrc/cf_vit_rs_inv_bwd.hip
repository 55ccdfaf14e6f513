// The vector-Jacobian product of the inverse transformer flow step: the DATA + INV form of k_vit_step_bwd_rs
// (cf_vit_rs_bwd.h), instantiated in a translation unit of its own so that the training forms keep compiling to what they
// were (profiles/vit_decode_grad.md), as cf_step_inv_bwd.hip does for the conv steps.  This unit holds the pack kernel of the
// front product's fragments and the entry points.
#include "cf_vit_rs_bwd.h"

namespace {

constexpr int kInvBwdWsFloats = 2 * RS26::NG_C * 256;

// fragments of diag(e^{logs}) Wm^-T in the OFF_CT order of k_vit_rs_pack_bwd: element ((rt * NG + gi) * 64 + lane) * 4 + e =
// e^{logs[a]} Wm^-1[b][a] with a = 16 rt + (lane & 15) (output row) and b = 4 (4 gi + e) + (lane >> 4) (contraction index).  The
// scale sits in the fragments, not in the kernel: there it would be one more 4-float load and four multiplies per lane on the
// critical path of a kernel that stands at its register limit, here it is 2 048 multiplies once per parameter version.
template <class V>
__global__ __launch_bounds__(256) void k_vit_rs_pack_inv_bwd(const float* __restrict__ winv, const float* __restrict__ logs,
                                                             float* __restrict__ wsv) {
    constexpr int C = V::C;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < 2 * V::NG_C * 256; i += gridDim.x * 256) {
        const int e = i & 3, lane = (i >> 2) & 63, q = i >> 8, gi = q % V::NG_C, rt = q / V::NG_C;
        const int a = 16 * rt + (lane & 15), b = 4 * (4 * gi + e) + (lane >> 4);
        wsv[i] = (a < C && b < C) ? expf(logs[a]) * winv[b * C + a] : 0.f;
    }
}

}  // namespace

extern "C" {

int64_t cf_vit_inv_step_bwd_ws_bytes(int C) { return C == 26 ? (int64_t)kInvBwdWsFloats * 4 : 0; }

// winv: the Wm^-1 (C, C) that cf_vit_step_prepare_batch(..., winv) produces; logs: the ActNorm's log-scales (C,)
int cf_vit_inv_step_bwd_prepare(const float* winv, const float* logs, void* wsv, int C, cf_stream_t stream) {
    CF_REQUIRE(winv && logs && wsv && (reinterpret_cast<uintptr_t>(wsv) & 15) == 0);
    if (C != 26) { cf_set_error("cf_vit_inv_step_bwd_prepare: C=%d unsupported", C); return CF_ERR_UNSUPPORTED; }
    k_vit_rs_pack_inv_bwd<RS26><<<dim3(kInvBwdWsFloats / 256), dim3(256), 0, cf_s(stream)>>>(winv, logs, (float*)wsv);
    CF_LAUNCH_CHECK();
    return 0;
}

// the vector-Jacobian product of the INVERSE step (Conv1x1^-1 o ActNorm^-1 o TransCoupling^-1) at its output: given x (B, C, 8, 1),
// the step input that the inverse recovered (batch stride x_bstride >= 8 C), and gx = d L / d x (dense), writes gz = d L / d z
// (dense) for the z the inverse was given.  Data only - no parameter gradient, no plane, no LayerNorm partial.  ws / wsb: the
// row-split forward tables and the backward kernel's (cf_vit_step_prepare_batch with form CF_VIT_FORM_RS and wsb); wsv:
// cf_vit_inv_step_bwd_prepare.  One launch of (B + 3) / 4 workgroups, no atomics: two calls give the same bits.
int cf_vit_inv_step_bwd_data(const float* x, const float* gx, const void* ws, const void* wsb, const void* wsv, float* gz, int B,
                             int C, int depth, int64_t x_bstride, cf_stream_t stream) {
    if (B == 0) return 0;
    CF_REQUIRE(x && gx && ws && wsb && wsv && gz && B > 0 && x_bstride >= (int64_t)C * 8);
    if (C != 26 || depth < 1 || depth > kVitMaxDepth) {
        cf_set_error("cf_vit_inv_step_bwd_data: C=%d depth=%d unsupported", C, depth);
        return CF_ERR_UNSUPPORTED;
    }
    constexpr size_t lds_bytes = (size_t)RB26::LDS_FLOATS * sizeof(float);
    static std::atomic<uint64_t> raised;
    const void* kernel = (const void*)k_vit_step_bwd_rs<RS26, false, true, true>;
    if (int rc_ = cf_raise_dynamic_lds(kernel, 160 * 1024, raised, __func__)) return rc_;
    const int nwg = (B + 3) / 4;
    // the kernel's upstream / result slots: it is given d/dx and writes d/dz; the log-det slot carries wsv
    k_vit_step_bwd_rs<RS26, false, true, true><<<dim3((unsigned)nwg), dim3(256), lds_bytes, cf_s(stream)>>>(
        x, gx, (const float*)wsv, gz, (const float*)ws, (const float*)wsb, nullptr, nullptr, B, nwg * 4, x_bstride, depth);
    CF_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
