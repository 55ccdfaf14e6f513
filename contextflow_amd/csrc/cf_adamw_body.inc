// Body of the AdamW kernels of cf_optim.hip, included once per kernel form so that every form is compiled from the same text.
// In scope at the include: tb, step, lr, lnb1, lnb2, beta2, w1, w2, eps, decay, maximize; CF_ADAMW_GRAD(ge) is the form's hook
// on a gradient element before use (empty for k_adamw).
// Why a textual fragment and not a __device__ __forceinline__ function templated on the hook: k_adamw's instructions must stay
// what they were before k_adamw_dev existed, and they do only in this form.  Checked on the device-only assembly of cf_optim.hip
// (hipcc -O3 --offload-arch=gfx950 --cuda-device-only -S, block labels renumbered) against the revision before: k_adamw's 488
// instructions are the same, line for line.  The function form was tried: same arithmetic, but the early return becomes a branch
// inside the kernel and hipcc builds the exec masks around the float4 / scalar split differently (490 instructions, ten scalar
// ones changed).  Repeat that comparison when this file changes.
// The second hook: CF_ADAMW_EMA(text) keeps the text of the parameter average (the ema column of the table,
// its pointer in the float4 alignment test, the update behind the stores of p, m, v in the float4 path and in the scalar path) and
// expands to its argument for k_adamw_ema / k_adamw_dev_ema<...> and to NOTHING for the three earlier kernels.  In scope for it:
// tb.ema, ema_decay (double), ema_warmup.  With it, by the same command and renumbering, the assembly of k_adamw, k_adamw_dev<true>
// and k_adamw_dev<false> equals, line for line and directives included, the assembly from the file without the hook (482, 493 and
// 486 instruction lines when directives, labels and comments are left out).
    const int wg = blockIdx.x;
    int lo = 0, hi = tb.count;           // tensor i with first[i] <= wg < first[i + 1]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tb.first[mid] <= wg) lo = mid; else hi = mid;
    }
    const int i = lo, n = tb.n[i];
    float* __restrict__ p = tb.p[i]; const float* __restrict__ g = tb.g[i];
    float* __restrict__ m = tb.m[i]; float* __restrict__ v = tb.v[i];
    const double t = (double)step[0];
    const double bc1 = 1.0 - exp(t * lnb1), bc2 = 1.0 - exp(t * lnb2);
    const float step_size = (float)(lr / bc1), bc2_sqrt = (float)sqrt(bc2);
    CF_ADAMW_EMA(
        float* __restrict__ ea = tb.ema[i];
        const bool ema_copy = t == 1.0;                             // the first update copies: no lerp with weight 1
        const double ema_d = ema_warmup ? fmin(ema_decay, (1.0 + t) / (10.0 + t)) : ema_decay;
        const float ema_w = (float)(1.0 - ema_d);
        // separately rounded difference, product and sum, so that every form and both paths give the same bits.  Plain operators
        // under contract(off), not __fsub_rn / __fmul_rn / __fadd_rn: hipcc's header defines those as plain operators compiled
        // under its default contraction, and the product and the sum came out as one v_pk_fma_f32 in the float4 path
        auto avg = [&](float& ee, float pe) {
            _Pragma("clang fp contract(off)")
            const float diff = pe - ee;
            const float prod = ema_w * diff;
            ee = ema_copy ? pe : ee + prod;
        };
    )
    auto upd = [&](float& pe, float ge, float& me, float& ve) {
        CF_ADAMW_GRAD(ge);
        if (maximize) ge = -ge;
        pe *= decay;
        me = me + w1 * (ge - me);                                   // exp_avg.lerp_(grad, 1 - beta1)
        ve = ve * beta2 + w2 * ge * ge;                             // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2)
        const float denom = sqrtf(ve) / bc2_sqrt + eps;
        pe = pe - step_size * (me / denom);                         // param.addcdiv_(exp_avg, denom, value = -step_size)
    };
    const int e0 = ((wg - tb.first[i]) * 256 + threadIdx.x) * 4;
    if (e0 >= n) return;
    const bool vec = e0 + 4 <= n && ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) |
                                      reinterpret_cast<uintptr_t>(v) CF_ADAMW_EMA(| reinterpret_cast<uintptr_t>(ea))) & 15) == 0;
    if (vec) {
        float4 pe = *reinterpret_cast<float4*>(p + e0), me = *reinterpret_cast<float4*>(m + e0), ve = *reinterpret_cast<float4*>(v + e0);
        const float4 ge = *reinterpret_cast<const float4*>(g + e0);
        upd(pe.x, ge.x, me.x, ve.x); upd(pe.y, ge.y, me.y, ve.y); upd(pe.z, ge.z, me.z, ve.z); upd(pe.w, ge.w, me.w, ve.w);
        *reinterpret_cast<float4*>(p + e0) = pe; *reinterpret_cast<float4*>(m + e0) = me; *reinterpret_cast<float4*>(v + e0) = ve;
        CF_ADAMW_EMA(
            float4 ee = *reinterpret_cast<float4*>(ea + e0);
            avg(ee.x, pe.x); avg(ee.y, pe.y); avg(ee.z, pe.z); avg(ee.w, pe.w);
            *reinterpret_cast<float4*>(ea + e0) = ee;
        )
    } else {
        for (int e = e0; e < n && e < e0 + 4; ++e) {
            float pe = p[e], me = m[e], ve = v[e];
            upd(pe, g[e], me, ve);
            p[e] = pe; m[e] = me; v[e] = ve;
            CF_ADAMW_EMA(float ee = ea[e]; avg(ee, pe); ea[e] = ee;)
        }
    }
