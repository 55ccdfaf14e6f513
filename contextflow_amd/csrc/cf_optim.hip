// AdamW update of the training step (model.py:289: optim.AdamW(model.parameters(), lr); experiment_cl.py:136 /
// experiment_ad.py:213: optimizer.step()) over MANY tensors in one launch.
//
// The flow's 135 (cifar10) ... 571 (smap) parameter tensors are tiny (9 ... 147 K elements): torch's fused multi-tensor kernel
// takes 4 (16) launches of 43 (15) us for them - 172 (250) us of a 1.44 (1.62) ms training step at the reference's batch of
// 256 - because a launch takes at most 48 tensors in 64 K-element chunks.  Here the tensor table travels in the kernel
// arguments (kAdamBatch entries per launch), a workgroup owns 1024 consecutive elements of one tensor (found by a binary search
// over the table's cumulative workgroup counts), 16-byte accesses: HBM-bound (7 floats per element; 9 in the forms that also keep
// an exponential moving average of the parameters, below), a few microseconds.
// Arithmetic = torch.optim.AdamW's, term by term, in fp32 (adamw.py::_single_tensor_adamw): decoupled weight decay, lerp form
// of the first moment, bias corrections from the step count read on the device (capturable: the count is a device scalar
// the caller increments before the launch).
#include "cf_common.h"
#include <math.h>
#include <type_traits>

namespace {

constexpr int kAdamBatch = 72;
struct AdamBatch {
    float* p[kAdamBatch];
    const float* g[kAdamBatch];
    float* m[kAdamBatch];
    float* v[kAdamBatch];
    int n[kAdamBatch];
    int first[kAdamBatch + 1];           // first workgroup of tensor i; first[count] = workgroups of the launch
    int count;
};

// w1 = 1 - beta1, w2 = 1 - beta2, decay = 1 - lr weight_decay are formed by the host in double, as torch forms them; the bias
// corrections 1 - beta^t in double on the device (t is only known there), from ln(beta): one exp per thread and moment.
// The body lives in cf_adamw_body.inc (a fragment included once per kernel, hence no header): k_adamw and k_adamw_dev below are
// compiled from the same text, and k_adamw's code is the one it had before k_adamw_dev existed (compared in the assembly; the
// fragment says how, and why it is no function).
__global__ __launch_bounds__(256) void k_adamw(const AdamBatch tb, const float* __restrict__ step, double lr, double lnb1, double lnb2,
                                               float beta2, float w1, float w2, float eps, float decay, int maximize) {
#define CF_ADAMW_GRAD(ge)
#define CF_ADAMW_EMA(...)
#include "cf_adamw_body.inc"
#undef CF_ADAMW_EMA
#undef CF_ADAMW_GRAD
}

// The same update with the learning rate read from the device (a captured launch then follows a schedule: the host fills the
// scalar between replays) and, SCALE, the gradient clipping of the step fused in.  decay = 1 - lr weight_decay in double, product
// and difference rounded separately (__dmul_rn: no fma), as the host forms it for k_adamw: equal lr => the bits of k_adamw.
// rec = {norm, coef} of k_grad_norm_finish.
template <bool SCALE>
__global__ __launch_bounds__(256) void k_adamw_dev(const AdamBatch tb, const float* __restrict__ step, const double* __restrict__ lr_dev,
                                                   const float* __restrict__ rec, double weight_decay, double lnb1, double lnb2, float beta2,
                                                   float w1, float w2, float eps, int maximize) {
    const double lr = lr_dev[0];
    const float decay = (float)(1.0 - __dmul_rn(lr, weight_decay));
    const float coef = SCALE ? rec[1] : 1.f;
    // SCALE: one fp32 rounding of the product, as g.mul_(coef) followed by the unscaled update gives (__fmul_rn: never contracted
    // into the first moment's subtraction)
#define CF_ADAMW_GRAD(ge) if (SCALE) ge = __fmul_rn(ge, coef)
#define CF_ADAMW_EMA(...)
#include "cf_adamw_body.inc"
#undef CF_ADAMW_EMA
#undef CF_ADAMW_GRAD
}

// ---- the same three forms with an exponential moving average of the parameters (Polyak weights) -------------------------------
// One more table column, ema[i]: after the parameter element is updated the same thread writes ema = p_new at t = 1 and
// ema += w (p_new - ema) afterwards, w = (float)(1 - d_t), d_t = ema_warmup ? min(ema_decay, (1 + t) / (10 + t)) : ema_decay in
// double from the step count the kernel reads anyway: a captured launch follows the warm-up of the decay.  9 floats per element
// instead of 7.  The table has 40 bytes of pointers per tensor: kAdamEmaBatch entries keep it (3080 bytes) with the scalars and the
// hidden arguments under the 4 KB of kernel arguments, as 72 entries of 32 do for AdamBatch (2888).
// The body's second hook, CF_ADAMW_EMA(text), keeps its text here and is empty above.
constexpr int kAdamEmaBatch = 64;
struct AdamEmaBatch {
    float* p[kAdamEmaBatch];
    const float* g[kAdamEmaBatch];
    float* m[kAdamEmaBatch];
    float* v[kAdamEmaBatch];
    float* ema[kAdamEmaBatch];
    int n[kAdamEmaBatch];
    int first[kAdamEmaBatch + 1];
    int count;
};
static_assert(sizeof(AdamEmaBatch) <= 3200, "AdamEmaBatch travels in the kernel arguments");

__global__ __launch_bounds__(256) void k_adamw_ema(const AdamEmaBatch tb, const float* __restrict__ step, double lr, double lnb1, double lnb2,
                                                   float beta2, float w1, float w2, float eps, float decay, int maximize, double ema_decay,
                                                   int ema_warmup) {
#define CF_ADAMW_GRAD(ge)
#define CF_ADAMW_EMA(...) __VA_ARGS__
#include "cf_adamw_body.inc"
#undef CF_ADAMW_EMA
#undef CF_ADAMW_GRAD
}

template <bool SCALE>
__global__ __launch_bounds__(256) void k_adamw_dev_ema(const AdamEmaBatch tb, const float* __restrict__ step, const double* __restrict__ lr_dev,
                                                       const float* __restrict__ rec, double weight_decay, double lnb1, double lnb2, float beta2,
                                                       float w1, float w2, float eps, int maximize, double ema_decay, int ema_warmup) {
    const double lr = lr_dev[0];
    const float decay = (float)(1.0 - __dmul_rn(lr, weight_decay));
    const float coef = SCALE ? rec[1] : 1.f;
#define CF_ADAMW_GRAD(ge) if (SCALE) ge = __fmul_rn(ge, coef)
#define CF_ADAMW_EMA(...) __VA_ARGS__
#include "cf_adamw_body.inc"
#undef CF_ADAMW_EMA
#undef CF_ADAMW_GRAD
}

// the launches of one table walk of every AdamW form: Batch = AdamBatch (ema is not looked at) or AdamEmaBatch; fn(table, workgroups)
template <typename Batch, typename F>
int adam_batches(int n, float* const* p, const float* const* g, float* const* m, float* const* v, float* const* ema, const int64_t* numel,
                 F&& fn) {
    constexpr int cap = (int)(sizeof(Batch::n) / sizeof(int));
    int i = 0;
    while (i < n) {
        Batch tb{};
        int wgs = 0, c = 0;
        for (; i < n && c < cap; ++i) {
            CF_REQUIRE(numel[i] >= 0 && numel[i] < (1ll << 31));
            if (numel[i] == 0) continue;
            CF_REQUIRE(p[i] && g[i] && m[i] && v[i]);
            tb.p[c] = p[i]; tb.g[c] = g[i]; tb.m[c] = m[i]; tb.v[c] = v[i]; tb.n[c] = (int)numel[i];
            if constexpr (std::is_same<Batch, AdamEmaBatch>::value) {
                CF_REQUIRE(ema[i]);
                tb.ema[c] = ema[i];
            }
            tb.first[c] = wgs;
            wgs += (int)((numel[i] + 1023) / 1024);
            ++c;
        }
        if (c == 0) break;
        tb.first[c] = wgs; tb.count = c;
        const int rc = fn(tb, wgs);
        if (rc != 0) return rc;
    }
    return 0;
}

// ---- exchange of the contents of many tensor pairs (optim.FusedAdamW.ema_scope: parameters against their averages) --------------
// The table form of the kernels above: 16 bytes of pointers per pair, a workgroup owns 1024 consecutive elements of one pair,
// float4 where both pointers are 16-byte aligned and four elements are left, scalar otherwise.  Every element is read and written
// by one thread: an exact exchange.
constexpr int kSwapBatch = 128;
struct SwapBatch {
    float* a[kSwapBatch];
    float* b[kSwapBatch];
    int n[kSwapBatch];
    int first[kSwapBatch + 1];
    int count;
};
static_assert(sizeof(SwapBatch) <= 3200, "SwapBatch travels in the kernel arguments");

__global__ __launch_bounds__(256) void k_swap(const SwapBatch tb) {
    const int wg = blockIdx.x;
    int lo = 0, hi = tb.count;           // pair i with first[i] <= wg < first[i + 1]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tb.first[mid] <= wg) lo = mid; else hi = mid;
    }
    const int i = lo, n = tb.n[i];
    float* a = tb.a[i]; float* b = tb.b[i];
    const int e0 = ((wg - tb.first[i]) * 256 + threadIdx.x) * 4;
    if (e0 >= n) return;
    if (e0 + 4 <= n && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0) {
        const float4 ae = *reinterpret_cast<float4*>(a + e0), be = *reinterpret_cast<float4*>(b + e0);
        *reinterpret_cast<float4*>(a + e0) = be; *reinterpret_cast<float4*>(b + e0) = ae;
    } else {
        for (int e = e0; e < n && e < e0 + 4; ++e) {
            const float ae = a[e], be = b[e];
            a[e] = be; b[e] = ae;
        }
    }
}

// ---- global gradient norm and clipping (experiment_cl.py:135 / experiment_ad.py:212: nn.utils.clip_grad_norm_) -----------------
// Sum of squares over many tensors in the form of k_adamw: the table (gradient pointer, element count, first workgroup: 16 bytes
// per tensor, kNormBatch per launch) travels in the kernel arguments, a workgroup owns 1024 consecutive elements of one tensor.
// Squares and sums are fp64 from the first product on (the kernel moves 4 bytes per element: HBM-bound either way); a wave
// reduces by shuffles, the four waves through LDS in wave order, lane 0 STORES the workgroup's partial - no atomics, so the
// summation order is fixed and a replayed step gives the bits of the eager one.
constexpr int kNormBatch = 224;
struct NormBatch {
    float* g[kNormBatch];
    int n[kNormBatch];
    int first[kNormBatch + 1];           // first workgroup of tensor i; first[count] = workgroups of the launch
    int count;
};

__device__ __forceinline__ int norm_tensor_of(const NormBatch& tb, int wg) {
    int lo = 0, hi = tb.count;           // tensor i with first[i] <= wg < first[i + 1]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tb.first[mid] <= wg) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k_grad_sumsq(const NormBatch tb, double* __restrict__ partials) {
    __shared__ double sw[4];
    const int wg = blockIdx.x;
    const int i = norm_tensor_of(tb, wg), n = tb.n[i];
    const float* __restrict__ g = tb.g[i];
    const int e0 = ((wg - tb.first[i]) * 256 + threadIdx.x) * 4;
    double s = 0.0;
    if (e0 < n) {
        if (e0 + 4 <= n && (reinterpret_cast<uintptr_t>(g) & 15) == 0) {
            const float4 ge = *reinterpret_cast<const float4*>(g + e0);
            const double x = ge.x, y = ge.y, z = ge.z, w = ge.w;
            s = x * x; s += y * y; s += z * z; s += w * w;
        } else {
            for (int e = e0; e < n && e < e0 + 4; ++e) {
                const double x = g[e];
                s += x * x;
            }
        }
    }
    s = cf_wave_sum_d(s);
    if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partials[wg] = ((sw[0] + sw[1]) + sw[2]) + sw[3];
}

// One workgroup: thread t sums partials[t], [t + 256], ... in that order, then the fixed block reduction.  rec[0] = norm,
// rec[1] = the coefficient of torch's clip_grad_norm_: c = max_norm / (norm + 1e-6) in fp32, clamped to 1 by a comparison that
// lets a NaN c through (torch.clamp propagates NaN; fminf would not): a non-finite norm poisons the update, as in torch with
// error_if_nonfinite = False.
__global__ __launch_bounds__(256) void k_grad_norm_finish(const double* __restrict__ partials, int count, float max_norm, float* __restrict__ rec) {
    __shared__ double sw[4];
    double s = 0.0;
    for (int k = threadIdx.x; k < count; k += 256) s += partials[k];
    s = cf_wave_sum_d(s);
    if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(((sw[0] + sw[1]) + sw[2]) + sw[3]);
        const float c = max_norm / (norm + 1e-6f);
        rec[0] = norm;
        rec[1] = c > 1.f ? 1.f : c;
    }
}

// g *= rec[1] in place (the standalone clip_grad_norm_): one fp32 product per element
__global__ __launch_bounds__(256) void k_grad_scale(const NormBatch tb, const float* __restrict__ rec) {
    const int wg = blockIdx.x;
    const int i = norm_tensor_of(tb, wg), n = tb.n[i];
    float* __restrict__ g = tb.g[i];
    const float coef = rec[1];
    const int e0 = ((wg - tb.first[i]) * 256 + threadIdx.x) * 4;
    if (e0 >= n) return;
    if (e0 + 4 <= n && (reinterpret_cast<uintptr_t>(g) & 15) == 0) {
        float4 ge = *reinterpret_cast<float4*>(g + e0);
        ge.x *= coef; ge.y *= coef; ge.z *= coef; ge.w *= coef;
        *reinterpret_cast<float4*>(g + e0) = ge;
    } else {
        for (int e = e0; e < n && e < e0 + 4; ++e) g[e] *= coef;
    }
}

// the launches of one table walk over n gradients: fn(table, workgroups, first partial of the launch)
template <typename F>
int norm_batches(int n, float* const* g, const int64_t* numel, F&& fn) {
    int i = 0;
    int64_t base = 0;
    while (i < n) {
        NormBatch tb{};
        int wgs = 0, c = 0;
        for (; i < n && c < kNormBatch; ++i) {
            if (numel[i] == 0) continue;
            tb.g[c] = g[i]; tb.n[c] = (int)numel[i];
            tb.first[c] = wgs;
            wgs += (int)((numel[i] + 1023) / 1024);
            ++c;
        }
        if (c == 0) break;
        tb.first[c] = wgs; tb.count = c;
        const int rc = fn(tb, wgs, base);
        if (rc != 0) return rc;
        base += wgs;
    }
    return 0;
}

}  // namespace

extern "C" {

int cf_adamw_step_batch(int n, float* const* p, const float* const* g, float* const* m, float* const* v, const int64_t* numel,
                        const float* step, double lr, double beta1, double beta2, double eps, double weight_decay, int maximize,
                        cf_stream_t stream) {
    CF_REQUIRE(n >= 0 && p && g && m && v && numel && step && lr >= 0. && beta1 >= 0. && beta1 < 1. && beta2 >= 0. && beta2 < 1. && eps >= 0.);
    return adam_batches<AdamBatch>(n, p, g, m, v, nullptr, numel, [&](const AdamBatch& tb, int wgs) {
        k_adamw<<<dim3(wgs), dim3(256), 0, cf_s(stream)>>>(tb, step, lr, beta1 > 0. ? log(beta1) : -1e300, beta2 > 0. ? log(beta2) : -1e300, (float)beta2,
                                                           (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps, (float)(1.0 - lr * weight_decay), maximize);
        CF_LAUNCH_CHECK();
        return 0;
    });
}

int cf_adamw_step_batch_dev(int n, float* const* p, const float* const* g, float* const* m, float* const* v, const int64_t* numel,
                            const float* step, const double* lr, const float* norm_rec, double beta1, double beta2, double eps,
                            double weight_decay, int maximize, cf_stream_t stream) {
    CF_REQUIRE(n >= 0 && p && g && m && v && numel && step && lr && beta1 >= 0. && beta1 < 1. && beta2 >= 0. && beta2 < 1. && eps >= 0.);
    const double lnb1 = beta1 > 0. ? log(beta1) : -1e300, lnb2 = beta2 > 0. ? log(beta2) : -1e300;
    return adam_batches<AdamBatch>(n, p, g, m, v, nullptr, numel, [&](const AdamBatch& tb, int wgs) {
        if (norm_rec)
            k_adamw_dev<true><<<dim3(wgs), dim3(256), 0, cf_s(stream)>>>(tb, step, lr, norm_rec, weight_decay, lnb1, lnb2, (float)beta2,
                                                                          (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps, maximize);
        else
            k_adamw_dev<false><<<dim3(wgs), dim3(256), 0, cf_s(stream)>>>(tb, step, lr, norm_rec, weight_decay, lnb1, lnb2, (float)beta2,
                                                                           (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps, maximize);
        CF_LAUNCH_CHECK();
        return 0;
    });
}

int cf_adamw_ema_step_batch(int n, float* const* p, const float* const* g, float* const* m, float* const* v, float* const* ema,
                            const int64_t* numel, const float* step, double lr, double beta1, double beta2, double eps, double weight_decay,
                            int maximize, double ema_decay, int ema_warmup, cf_stream_t stream) {
    CF_REQUIRE(n >= 0 && p && g && m && v && numel && step && lr >= 0. && beta1 >= 0. && beta1 < 1. && beta2 >= 0. && beta2 < 1. && eps >= 0.);
    CF_REQUIRE(ema && ema_decay >= 0. && ema_decay < 1.);
    return adam_batches<AdamEmaBatch>(n, p, g, m, v, ema, numel, [&](const AdamEmaBatch& tb, int wgs) {
        k_adamw_ema<<<dim3(wgs), dim3(256), 0, cf_s(stream)>>>(tb, step, lr, beta1 > 0. ? log(beta1) : -1e300, beta2 > 0. ? log(beta2) : -1e300,
                                                               (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps,
                                                               (float)(1.0 - lr * weight_decay), maximize, ema_decay, ema_warmup != 0);
        CF_LAUNCH_CHECK();
        return 0;
    });
}

int cf_adamw_ema_step_batch_dev(int n, float* const* p, const float* const* g, float* const* m, float* const* v, float* const* ema,
                                const int64_t* numel, const float* step, const double* lr, const float* norm_rec, double beta1, double beta2,
                                double eps, double weight_decay, int maximize, double ema_decay, int ema_warmup, cf_stream_t stream) {
    CF_REQUIRE(n >= 0 && p && g && m && v && numel && step && lr && beta1 >= 0. && beta1 < 1. && beta2 >= 0. && beta2 < 1. && eps >= 0.);
    CF_REQUIRE(ema && ema_decay >= 0. && ema_decay < 1.);
    const double lnb1 = beta1 > 0. ? log(beta1) : -1e300, lnb2 = beta2 > 0. ? log(beta2) : -1e300;
    return adam_batches<AdamEmaBatch>(n, p, g, m, v, ema, numel, [&](const AdamEmaBatch& tb, int wgs) {
        if (norm_rec)
            k_adamw_dev_ema<true><<<dim3(wgs), dim3(256), 0, cf_s(stream)>>>(tb, step, lr, norm_rec, weight_decay, lnb1, lnb2, (float)beta2,
                                                                              (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps, maximize,
                                                                              ema_decay, ema_warmup != 0);
        else
            k_adamw_dev_ema<false><<<dim3(wgs), dim3(256), 0, cf_s(stream)>>>(tb, step, lr, norm_rec, weight_decay, lnb1, lnb2, (float)beta2,
                                                                               (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps, maximize,
                                                                               ema_decay, ema_warmup != 0);
        CF_LAUNCH_CHECK();
        return 0;
    });
}

int cf_swap_batch(int n, float* const* a, float* const* b, const int64_t* numel, cf_stream_t stream) {
    CF_REQUIRE(n >= 0 && (n == 0 || (a && b && numel)));
    for (int i = 0; i < n; ++i) CF_REQUIRE(numel[i] >= 0 && numel[i] < (1ll << 31) && (numel[i] == 0 || (a[i] && b[i] && a[i] != b[i])));
    int i = 0;
    while (i < n) {
        SwapBatch tb{};
        int wgs = 0, c = 0;
        for (; i < n && c < kSwapBatch; ++i) {
            if (numel[i] == 0) continue;
            tb.a[c] = a[i]; tb.b[c] = b[i]; tb.n[c] = (int)numel[i];
            tb.first[c] = wgs;
            wgs += (int)((numel[i] + 1023) / 1024);
            ++c;
        }
        if (c == 0) break;
        tb.first[c] = wgs; tb.count = c;
        k_swap<<<dim3(wgs), dim3(256), 0, cf_s(stream)>>>(tb);
        CF_LAUNCH_CHECK();
    }
    return 0;
}

int64_t cf_grad_norm_partials(int n, const int64_t* numel) {
    if (n < 0 || (n > 0 && !numel)) return CF_ERR_ARG;
    int64_t wgs = 0;
    for (int i = 0; i < n; ++i) {
        if (numel[i] < 0) return CF_ERR_ARG;
        wgs += (numel[i] + 1023) / 1024;
    }
    return wgs;
}

int cf_grad_norm_batch(int n, const float* const* g, const int64_t* numel, double max_norm, double* partials, int64_t partials_cap,
                       float* norm_rec, cf_stream_t stream) {
    CF_REQUIRE(n >= 0 && (n == 0 || (g && numel)) && partials && norm_rec && max_norm > 0.);
    int64_t total = 0;
    for (int i = 0; i < n; ++i) {
        CF_REQUIRE(numel[i] >= 0 && numel[i] < (1ll << 31) && (numel[i] == 0 || g[i]));
        total += (numel[i] + 1023) / 1024;
    }
    CF_REQUIRE(total <= partials_cap && total < (1ll << 31));
    const int rc = norm_batches(n, const_cast<float* const*>(g), numel, [&](const NormBatch& tb, int wgs, int64_t base) {
        k_grad_sumsq<<<dim3(wgs), dim3(256), 0, cf_s(stream)>>>(tb, partials + base);
        CF_LAUNCH_CHECK();
        return 0;
    });
    if (rc != 0) return rc;
    k_grad_norm_finish<<<dim3(1), dim3(256), 0, cf_s(stream)>>>(partials, (int)total, (float)max_norm, norm_rec);
    CF_LAUNCH_CHECK();
    return 0;
}

int cf_grad_scale_batch(int n, float* const* g, const int64_t* numel, const float* norm_rec, cf_stream_t stream) {
    CF_REQUIRE(n >= 0 && (n == 0 || (g && numel)) && norm_rec);
    for (int i = 0; i < n; ++i) CF_REQUIRE(numel[i] >= 0 && numel[i] < (1ll << 31) && (numel[i] == 0 || g[i]));
    return norm_batches(n, g, numel, [&](const NormBatch& tb, int wgs, int64_t) {
        k_grad_scale<<<dim3(wgs), dim3(256), 0, cf_s(stream)>>>(tb, norm_rec);
        CF_LAUNCH_CHECK();
        return 0;
    });
}

}  // extern "C"
