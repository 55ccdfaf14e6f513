// Context-conditioned (specialist) branches of the flow layers: every Conv1x1 / ActNorm /
// Coupling of a specialist model owns a context encoder and a small CN net whose output turns the layer's parameters
// into PER-SAMPLE parameters; the priors get per-sample shifts of their component means / scales.
//
// All of it is HBM- / VALU-bound work over (sample, channel, pixel); the CN nets themselves are cf_linear (MFMA).
// One workgroup owns one sample in the three per-sample kernels, so the per-sample parameters live in LDS / registers.
#include "cf_common.h"
#include <math.h>
#include <algorithm>
#include <type_traits>

namespace {


// ContextEncoder = (OneHotEncoder | EyeEncoder) -> UniformCatDequantization (rtdl/nn/_embeddings.py:76-150,
// dequantize.py:55-64): out[b, j] = (x[b, j] + u[b, j]) / qbins[j]; x = the integer context itself (eye) or its
// one-hot code, column j belonging to the context variable whose cardinality range contains j.
__global__ __launch_bounds__(256) void k_ctx_encode(const int64_t* __restrict__ ctx, const float* __restrict__ u,
                                                    const float* __restrict__ qbins, const int64_t* __restrict__ card,
                                                    float* __restrict__ out, int B, int nctx, int width, int onehot) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)B * width) return;
    const int b = (int)(e / width), j = (int)(e - (int64_t)b * width);
    float x;
    if (onehot) {                                     // modes 1 (one-hot) and 2 (binary sign code): find the variable
        int i = 0, off = 0;
        while (i < nctx - 1 && j >= off + (int)card[i]) { off += (int)card[i]; ++i; }
        if (onehot == 2) {
            // ArgmaxCatDequantization (dequantize.py:236-262): big-endian binary code of every context variable
            // (card[i] = its number of bits), one zero pad column when the total is odd; z = u * (2 bit - 1)
            const int nb = (int)card[i], k = j - off;
            const int bit = (k < nb) ? (int)((ctx[(int64_t)b * nctx + i] >> (nb - 1 - k)) & 1) : 0;
            out[e] = u[e] * (bit ? 1.f : -1.f);
            return;
        }
        x = (ctx[(int64_t)b * nctx + i] == (int64_t)(j - off)) ? 1.f : 0.f;
    } else {
        x = (float)ctx[(int64_t)b * nctx + j];
    }
    out[e] = (x + u[e]) / qbins[j];
}

// row stride of the transposed per-sample matrix in LDS: C rounded up to 8 (16-byte rows for the float4 reads), plus 4
// when that is a multiple of 32 (the transposed writes would otherwise all land in one bank)
__host__ __device__ inline int conv1x1_ctx_cp(int C) {
    const int cp = (C + 7) & ~7;
    return (cp & 31) == 0 ? cp + 4 : cp;
}

// global -> LDS copy of n contiguous floats by the 256 threads of a workgroup, in batches of 8 independent loads per
// thread (16-byte loads when n and the source allow): a `dst[e] = src[e]` loop with a runtime bound is compiled to one
// dependent load -> store round trip per element, which makes these one-workgroup-per-sample kernels latency-bound.
__device__ __forceinline__ void stage_copy(float* __restrict__ dst, const float* __restrict__ src, int n, int tid) {
    if ((n & 3) == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
        const int n4 = n >> 2;
        const float4* s4 = reinterpret_cast<const float4*>(src);
        float4* d4 = reinterpret_cast<float4*>(dst);
        for (int e0 = tid; e0 < n4; e0 += 8 * 256) {
            float4 v[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = s4[min(e0 + i * 256, n4 - 1)];
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (e0 + i * 256 < n4) d4[e0 + i * 256] = v[i];
        }
    } else {
        for (int e0 = tid; e0 < n; e0 += 8 * 256) {
            float v[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = src[min(e0 + i * 256, n - 1)];
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (e0 + i * 256 < n) dst[e0 + i * 256] = v[i];
        }
    }
}

// ---- the per-sample matrix: element (o, i) of W_b = tril(m, -1) + diag(exp(diag m)) [+ NN - I] from v = m[o][i] and
// wm = NN[o][i] (nn: under contextflow).  Two arithmetic families that round differently ON PURPOSE - every kernel keeps the bits
// it has always produced, so the two orders must not be unified:
//   LDS kernels:  base + (wm - delta)          base = v | exp(v) | 0 below / on / above the diagonal, delta = (o == i)
//   wave kernels: (exp(v) - 1) + wm on the diagonal, v + wm elsewhere.  wb_element_wave is the first term, for the fragments on
//                 the block diagonal; the fragments below it hold m as it is, those above 0, and the caller adds NN to all.
//                 It also adds the diagonal's v to dsum (the log-det term of the forward; the backward has no use for it)
__device__ __forceinline__ float wb_element(float v, float wm, bool nn, int o, int i) {
    float w = o > i ? v : (o == i ? expf(v) : 0.f);
    if (nn) w += wm - (o == i ? 1.f : 0.f);
    return w;
}
__device__ __forceinline__ float wb_element_wave(float v, bool nn, int o, int i, float& dsum) {
    const float ex = expf(v) - (nn ? 1.f : 0.f);
    if (o == i) dsum += v;
    return o > i ? v : (o == i ? ex : 0.f);
}

// Squeeze((2,2)) (squeeze.py:10-11): offset of (channel c, pixel p) of the squeezed (C, H, W) sample inside the un-squeezed
// (C/4, 2H, 2W) one - the reads of a fused Squeeze in front of the pair, the writes of its adjoint
__device__ __forceinline__ int squeeze_index(int c, int p, int W, int HW) {
    const int yy = p / W, xx = p - yy * W;
    return (c >> 2) * 4 * HW + (2 * yy + ((c >> 1) & 1)) * 2 * W + 2 * xx + (c & 1);
}

// The two LDS forms of W_b, built by the 256 threads of a workgroup.  Both fetch what they read from global memory in batches
// of 8 independent loads at a clamped index (see stage_copy: a load inside the element loop costs one full memory latency per
// element) and zero the padding up to CP.
// Forward: Wt[i * CP + o] = W_b[o][i] from this sample's m staged in LDS (ms).  Lanes walk i: ms read without bank conflicts,
// Wt written at stride CP.  Returns dsum + weight * (this lane's share of sum diag m).
__device__ __forceinline__ float build_wb_transposed(float* Wt, const float* ms, const float* Wm, int C, int CP, float weight,
                                                     float dsum, int tid) {
    for (int e0 = tid; e0 < CP * C; e0 += 8 * 256) {
        float wm[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) wm[k] = Wm != nullptr ? Wm[min(e0 + k * 256, C * C - 1)] : 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int e = e0 + k * 256;
            if (e < CP * C) {
                const int o = e / C, i = e - o * C;
                float w = 0.f;
                if (o < C) {
                    const float v = ms[e];
                    w = wb_element(v, wm[k], Wm != nullptr, o, i);
                    if (o == i) dsum = fmaf(weight, v, dsum);
                }
                Wt[i * CP + o] = w;
            }
        }
    }
    return dsum;
}
// Backward: Wb[o * CP + i] = W_b[o][i] [* rowscale[o] (SCALE)] from this sample's m in global memory (mb).
template <bool SCALE>
__device__ __forceinline__ void build_wb_rowmajor(float* Wb, const float* mb, const float* Wm, const float* rowscale, int C, int CP,
                                                  int tid) {
    for (int e0 = tid; e0 < C * CP; e0 += 8 * 256) {
        float mv[8], wm[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int e = min(e0 + k * 256, C * CP - 1), o = e / CP, i = min(e - o * CP, C - 1);
            mv[k] = mb[o * C + i];
            wm[k] = Wm != nullptr ? Wm[o * C + i] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int e = e0 + k * 256;
            if (e < C * CP) {
                const int o = e / CP, i = e - o * CP;
                float w = 0.f;
                if (i < C) {
                    w = wb_element(mv[k], wm[k], Wm != nullptr, o, i);
                    if constexpr (SCALE) w *= rowscale[o];
                }
                Wb[e] = w;
            }
        }
    }
}

// The product of all four LDS kernels: out[c][p] = sum_k A[k * CP + c] v[k * vs + p], k < C.  A thread owns one pixel p and 8
// channels c0 .. c0 + 7 at a time - per k one read of v and two 16-byte (broadcast) reads of A - and hands each of its
// sums to epi(c, p, acc).
template <class Epi>
__device__ __forceinline__ void pixel8_product(const float* A, const float* v, int C, int CP, int vs, int HW, int tid, Epi epi) {
    const int ncb = CP >> 3;
    for (int e = tid; e < ncb * HW; e += 256) {
        const int cb = e / HW, p = e - cb * HW, c0 = cb * 8;
        float acc[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] = 0.f;
        for (int k = 0; k < C; ++k) {
            const float xv = v[k * vs + p];
            const float4 w0 = *reinterpret_cast<const float4*>(&A[k * CP + c0]);
            const float4 w1 = *reinterpret_cast<const float4*>(&A[k * CP + c0 + 4]);
            acc[0] = fmaf(w0.x, xv, acc[0]); acc[1] = fmaf(w0.y, xv, acc[1]);
            acc[2] = fmaf(w0.z, xv, acc[2]); acc[3] = fmaf(w0.w, xv, acc[3]);
            acc[4] = fmaf(w1.x, xv, acc[4]); acc[5] = fmaf(w1.y, xv, acc[5]);
            acc[6] = fmaf(w1.z, xv, acc[6]); acc[7] = fmaf(w1.w, xv, acc[7]);
        }
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (c0 + k < C) epi(c0 + k, p, acc[k]);
    }
}

// ActNorm with a context net: t_b, exp(-l_b) and l_b of channel c of sample b from m = CN(c) = [t_b | logs_b] per sample, plus
// the shared NN_t / NN_logs under contextflow (both given or neither).  WITH_T = false: the data backward has no use for t_b and
// no t to read.
struct ActNormCtxTerms { float t, s, l; };
template <bool WITH_T = true>
__device__ __forceinline__ ActNormCtxTerms actnorm_ctx_terms(const float* m, int b, const float* t, const float* logs, int C, int c) {
    float tv = 0.f;
    if constexpr (WITH_T) tv = m[(int64_t)b * 2 * C + c];
    float lv = m[(int64_t)b * 2 * C + C + c];
    if ((WITH_T ? t : logs) != nullptr) {
        if constexpr (WITH_T) tv += t[c];
        lv += logs[c];
    }
    return {tv, expf(-lv), lv};
}

// dyn[] of the two forward LDS kernels: the arrays in their order, sizes in floats.  The kernel carves dyn[] with these
// sizes (on dyn itself: the compiler must see LDS addresses), the launcher requests floats().  NACT = C with the ActNorm
// terms of k_affine_ctx, 0 without.  scr lies inside the dynamic block: no static LDS next to a 160 KiB request.
struct CtxFwdLds {
    int CP;
    int nWt;      // Wt[i][o] = W_b[o][i], row stride CP
    int nxs;      // xs[C][HW]  (16-byte aligned: C * CP is a multiple of 4)
    int nact;     // after scr[nscr]: tb[NACT] = t_b, sb[NACT] = exp(-logs_b)
    int nms;      // ms[C*C] this sample's CN(c) output, staged before the transposed read
    __host__ __device__ CtxFwdLds(int C, int HW, int NACT) : CP(conv1x1_ctx_cp(C)), nWt(C * CP), nxs(C * HW), nact(NACT), nms(C * C) {}
    static constexpr int nscr = 4;
    __host__ __device__ int floats() const { return nWt + nxs + nscr + 2 * nact + nms; }
};

// Conv1x1 with a context net (conv1x1.py:34-50): m = CN(c) reshaped (C, C) per sample;
//   W_b = tril(m, -1) + diag(exp(diag m))            [+ NN - I under contextflow]
//   z[b] = W_b x[b] per pixel;  ldj[b] = H W sum(diag m)   (the caller adds H W log|det NN| under contextflow -
//   the reference's own expression, not the log-det of W_b).
// One workgroup per sample: W_b^T (row stride CP = C rounded up to 8, zero padded) and x in LDS, then pixel8_product over the
// output channels.
__global__ __launch_bounds__(256) void k_conv1x1_ctx(const float* __restrict__ x, const float* __restrict__ m,
                                                     const float* __restrict__ Wm, float* __restrict__ z,
                                                     float* __restrict__ ldj, int C, int HW, int64_t xbs) {
    extern __shared__ __align__(16) float dyn[];
    const CtxFwdLds L(C, HW, 0);
    float *Wt = dyn, *xs = Wt + L.nWt, *scr = xs + L.nxs, *ms = scr + L.nscr;
    const int b = blockIdx.x, tid = threadIdx.x;
    stage_copy(ms, m + (int64_t)b * C * C, C * C, tid);
    __syncthreads();
    float dsum = build_wb_transposed(Wt, ms, Wm, C, L.CP, 1.f, 0.f, tid);
    stage_copy(xs, x + (int64_t)b * xbs, C * HW, tid);
    dsum = cf_block_sum<4>(dsum, scr);                // also the barrier that publishes Wt / xs
    if (tid == 0) ldj[b] = dsum * (float)HW;
    float* zb = z + (int64_t)b * C * HW;
    pixel8_product(Wt, xs, C, L.CP, HW, HW, tid, [=](int o, int p, float acc) { zb[(int64_t)o * HW + p] = acc; });
}

// ActNorm with a context net (actnorm.py:40-60): m = CN(c) = [t_b | logs_b] per sample (+ the shared NN_t / NN_logs
// under contextflow); z = (x - t_b) exp(-logs_b); ldj[b] = sum_c logs_b (reference quirk: no H W factor).
__global__ __launch_bounds__(256) void k_actnorm_ctx(const float* __restrict__ x, const float* __restrict__ m,
                                                     const float* __restrict__ t, const float* __restrict__ logs,
                                                     float* __restrict__ z, float* __restrict__ ldj, int C, int HW,
                                                     int64_t xbs) {
    __shared__ float tb[128], sb[128];
    __shared__ float scr[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    float lsum = 0.f;
    if (tid < C) {
        const ActNormCtxTerms a = actnorm_ctx_terms(m, b, t, logs, C, tid);
        tb[tid] = a.t; sb[tid] = a.s;
        lsum = a.l;
    }
    lsum = cf_block_sum<4>(lsum, scr);
    if (tid == 0) ldj[b] = lsum;
    const float* xb = x + (int64_t)b * xbs;
    float* zb = z + (int64_t)b * C * HW;
    for (int e = tid; e < C * HW; e += 256) { const int c = e / HW; zb[e] = (xb[e] - tb[c]) * sb[c]; }
}

// Conv1x1 and ActNorm of a specialist step in ONE pass over the sample (evaluation): z = (W_b x - t_b) exp(-logs_b) with
// W_b as in k_conv1x1_ctx (m1 = Conv1x1.CN(c), (B, C*C)) and t_b / logs_b as in k_actnorm_ctx (m2 = ActNorm.CN(c'), (B, 2C)).
// SQ: x is the un-squeezed (C/4, 2H, 2W) sample and Squeeze((2,2)) (squeeze.py:10-11) is folded into the staging reads.
//   ldj[b] (+)= H W (sum diag m1 + lad[0]) + sum_c logs_b + cadd       lad: log|det NN| (device scalar) or NULL
// One workgroup per sample, as the two kernels it replaces: one read of x, one write of z instead of two of each (+ the
// Squeeze copy), no intermediate tensor.
template <bool SQ>
__global__ __launch_bounds__(256) void k_affine_ctx(const float* __restrict__ x, const float* __restrict__ m1,
                                                    const float* __restrict__ Wm, const float* __restrict__ m2,
                                                    const float* __restrict__ t, const float* __restrict__ logs,
                                                    const float* __restrict__ lad, float cadd, float* __restrict__ z,
                                                    float* __restrict__ ldj, int C, int H, int W, int64_t xbs, int accumulate) {
    extern __shared__ __align__(16) float dyn[];
    const int HW = H * W;
    const CtxFwdLds L(C, HW, C);
    float *Wt = dyn, *xs = Wt + L.nWt, *scr = xs + L.nxs, *tb = scr + L.nscr, *sb = tb + L.nact, *ms = sb + L.nact;
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* xb = x + (int64_t)b * xbs;
    stage_copy(ms, m1 + (int64_t)b * C * C, C * C, tid);
    float dsum = 0.f;
    if (tid < C) {
        const ActNormCtxTerms a = actnorm_ctx_terms(m2, b, t, logs, C, tid);
        tb[tid] = a.t; sb[tid] = a.s;
        dsum = a.l;                                  // joins the block sum below with weight 1 (the diagonal gets H W)
    }
    if constexpr (!SQ) {
        stage_copy(xs, xb, C * HW, tid);
    } else {
        for (int e0 = tid; e0 < C * HW; e0 += 8 * 256) {
            float v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int e = min(e0 + k * 256, C * HW - 1), c = e / HW;
                v[k] = xb[squeeze_index(c, e - c * HW, W, HW)];
            }
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (e0 + k * 256 < C * HW) xs[e0 + k * 256] = v[k];
        }
    }
    __syncthreads();
    const float hw = (float)HW;
    dsum = build_wb_transposed(Wt, ms, Wm, C, L.CP, hw, dsum, tid);
    dsum = cf_block_sum<4>(dsum, scr);                // also the barrier that publishes Wt
    if (tid == 0) {
        const float v = dsum + (lad != nullptr ? hw * lad[0] : 0.f) + cadd;
        ldj[b] = accumulate ? ldj[b] + v : v;
    }
    float* zb = z + (int64_t)b * C * HW;
    pixel8_product(Wt, xs, C, L.CP, HW, HW, tid, [=](int o, int p, float acc) { zb[(int64_t)o * HW + p] = (acc - tb[o]) * sb[o]; });
}

typedef float f32x4 __attribute__((ext_vector_type(4)));

// What k_affine_ctx_wave and its transpose k_affine_ctx_bwd_wave (below) share: the fragment grid of a (C, W, W) level, the
// rows of a fused Squeeze((2,2)) and the ActNorm terms in the layout of the D rows.  Lane (n = lane & 15, kk = lane >> 4).
template <int C, int W>
struct AffineWave {
    static constexpr int HW = W * W, RT = C / 16, NG = C / 16, WIDE = HW >= 64, NT = WIDE ? HW / 64 : 1, NJ = WIDE ? 4 : 1;
    // the pixel of column n of pixel tile T; WIDE: the first of 4 pixels of one image row (W >= 4), one per column tile
    static __device__ __forceinline__ int pixel0(int T, int n) { return WIDE ? 64 * T + 4 * n : n; }
    // un-squeezed (C/4, 2W, 2W) sample: where row 2 yy + dy of channel q meets squeezed pixel (yy, xx) - the 2 floats there
    // are its phases (dy, dx = 0 | 1), squeezed channels 4 q + 2 dy + dx; WIDE: 8 floats, pixels (yy, xx .. xx + 3)
    template <class P>
    static __device__ __forceinline__ P phase_row(P sample, int q, int dy, int yy, int xx) {
        return sample + q * 4 * HW + (2 * yy + dy) * 2 * W + 2 * xx;
    }
    // t_b and l_b of rows o0 .. o0 + 3 of sample b, as actnorm_ctx_terms
    template <bool WITH_T = true>
    static __device__ __forceinline__ void actnorm_rows(const float* m2, int b, const float* t, const float* logs, int o0, float4& tv,
                                                        float4& lv) {
        if constexpr (WITH_T) tv = *reinterpret_cast<const float4*>(m2 + (int64_t)b * 2 * C + o0);
        lv = *reinterpret_cast<const float4*>(m2 + (int64_t)b * 2 * C + C + o0);
        if ((WITH_T ? t : logs) != nullptr) {
            if constexpr (WITH_T) {
                const float4 t0 = *reinterpret_cast<const float4*>(t + o0);
                tv.x += t0.x; tv.y += t0.y; tv.z += t0.z; tv.w += t0.w;
            }
            const float4 l0 = *reinterpret_cast<const float4*>(logs + o0);
            lv.x += l0.x; lv.y += l0.y; lv.z += l0.z; lv.w += l0.w;
        }
    }
};

// The same on the matrix pipe for the three levels of the image flows, ONE WAVE per sample and no LDS: per sample the
// product is (C x C) (C x HW) = 64 v_mfma_f32_16x16x4_f32 whatever the level, and every operand is read from global memory
// exactly once, in the MFMA's own register layout:
//   A (W_b, 16 rows x 4 k per instruction): lane (n = lane & 15, kk = lane >> 4) loads the float4 m1[o = 16 rt + n][16 g + 4 kk ..]
//     and uses its 4 values for 4 successive k-steps - the k order of a product is free as long as A and B agree;
//   B (x): for those k-steps lane (n, kk) needs x[i = 16 g + 4 kk + e][pixel of column n].  With 64 pixels or more, column n of
//     column tile j IS pixel 4 n + j: one float4 of x serves the four column tiles, and the four results of a row come
//     back as one float4 store.  On 4x4 images (16 pixels) the column is the pixel: dword loads, 64-byte runs.
//   SQ: i = 4 q + 2 dy + dx with q = 4 g + kk, e = 2 dy + dx - the four k-steps of a lane are the four phases of ONE channel
//     of the un-squeezed tensor: rows 2 y, 2 y + 1, 8 (2) consecutive floats each.
// tril / exp(diag) / + NN - I are applied to the A fragments in registers; t_b, logs_b come as float4 per (row tile, kk).
// BLK: m1 holds only the 16 x 16 blocks on and below the diagonal of the per-sample matrix, block (rt, g <= rt) at
// (rt (rt + 1) / 2 + g) * 256, row-major inside (the caller permutes the rows of Conv1x1.CN accordingly): the blocks above the
// diagonal are never needed, and a fragment load is 1 KB of contiguous memory instead of 16 runs of 64 bytes.
template <int C, int W, bool SQ, bool BLK>
__global__ __launch_bounds__(256) void k_affine_ctx_wave(const float* __restrict__ x, const float* __restrict__ m1,
                                                         const float* __restrict__ Wm, const float* __restrict__ m2,
                                                         const float* __restrict__ t, const float* __restrict__ logs,
                                                         const float* __restrict__ lad, float cadd, float* __restrict__ z,
                                                         float* __restrict__ ldj, int B, int64_t xbs, int accumulate) {
    using G = AffineWave<C, W>;
    constexpr int HW = G::HW, RT = G::RT, NG = G::NG, WIDE = G::WIDE, NT = G::NT, NJ = G::NJ;
    const int lane = threadIdx.x & 63, n = lane & 15, kk = lane >> 4;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;                                // a whole wave: the kernel has no barrier
    constexpr int NBLK = RT * (RT + 1) / 2;
    const float* mb = m1 + (int64_t)b * (BLK ? NBLK * 256 : C * C);
    const float* xb = x + (int64_t)b * xbs;
    // ---- A fragments.  W_b is block lower triangular on the 16 x 16 grid of fragments: blocks above the diagonal hold NN alone
    // (never read from m1), blocks below m1 + NN, the diagonal blocks the element-wise tril / exp(diag) / - I.
    float4 a[RT][NG];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int g = 0; g < NG; ++g)
            a[rt][g] = g <= rt ? *reinterpret_cast<const float4*>(BLK ? mb + (rt * (rt + 1) / 2 + g) * 256 + n * 16 + 4 * kk
                                                                        : mb + (16 * rt + n) * C + 16 * g + 4 * kk)
                               : make_float4(0.f, 0.f, 0.f, 0.f);
    float dsum = 0.f;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const int o = 16 * rt + n, i0 = 16 * g + 4 * kk;
            float v[4] = {a[rt][g].x, a[rt][g].y, a[rt][g].z, a[rt][g].w};
            if (g == rt) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = wb_element_wave(v[e], Wm != nullptr, o, i0 + e, dsum);
            }
            if (Wm != nullptr) {
                const float4 wv = *reinterpret_cast<const float4*>(Wm + o * C + i0);
                v[0] += wv.x; v[1] += wv.y; v[2] += wv.z; v[3] += wv.w;
            }
            a[rt][g] = make_float4(v[0], v[1], v[2], v[3]);
        }
    // ---- the product
    f32x4 acc[RT][NT][NJ];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int T = 0; T < NT; ++T)
#pragma unroll
            for (int j = 0; j < NJ; ++j) acc[rt][T][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int T = 0; T < NT; ++T)
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            float xv[4][NJ];                           // [k-step e][column tile j]
            if constexpr (WIDE) {
                if constexpr (!SQ) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float4 v = *reinterpret_cast<const float4*>(xb + (16 * g + 4 * kk + e) * HW + 64 * T + 4 * n);
                        xv[e][0] = v.x; xv[e][1] = v.y; xv[e][2] = v.z; xv[e][3] = v.w;
                    }
                } else {
                    const int p0 = G::pixel0(T, n), yy = p0 / W, xx = p0 - yy * W;
#pragma unroll
                    for (int dy = 0; dy < 2; ++dy) {
                        const float* row = G::phase_row(xb, 4 * g + kk, dy, yy, xx);
                        const float4 u0 = *reinterpret_cast<const float4*>(row), u1 = *reinterpret_cast<const float4*>(row + 4);
                        xv[2 * dy][0] = u0.x; xv[2 * dy][1] = u0.z; xv[2 * dy][2] = u1.x; xv[2 * dy][3] = u1.z;
                        xv[2 * dy + 1][0] = u0.y; xv[2 * dy + 1][1] = u0.w; xv[2 * dy + 1][2] = u1.y; xv[2 * dy + 1][3] = u1.w;
                    }
                }
            } else {
                if constexpr (!SQ) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) xv[e][0] = xb[(16 * g + 4 * kk + e) * HW + n];
                } else {
                    const int p0 = G::pixel0(T, n), yy = p0 / W, xx = p0 - yy * W;
#pragma unroll
                    for (int dy = 0; dy < 2; ++dy) {
                        const float2 u = *reinterpret_cast<const float2*>(G::phase_row(xb, 4 * g + kk, dy, yy, xx));
                        xv[2 * dy][0] = u.x; xv[2 * dy + 1][0] = u.y;
                    }
                }
            }
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                const float av[4] = {a[rt][g].x, a[rt][g].y, a[rt][g].z, a[rt][g].w};
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int j = 0; j < NJ; ++j)
                        acc[rt][T][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], xv[e][j], acc[rt][T][j], 0, 0, 0);
            }
        }
    // ---- ActNorm epilogue: rows o = 16 rt + 4 kk + r of this lane
    float* zb = z + (int64_t)b * C * HW;
    float lsum = 0.f;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        const int o0 = 16 * rt + 4 * kk;
        float4 tv, lv;
        G::actnorm_rows(m2, b, t, logs, o0, tv, lv);
        if (n == 0) lsum += (lv.x + lv.y) + (lv.z + lv.w);
        const float tt[4] = {tv.x, tv.y, tv.z, tv.w};
        const float ss[4] = {expf(-lv.x), expf(-lv.y), expf(-lv.z), expf(-lv.w)};
#pragma unroll
        for (int T = 0; T < NT; ++T)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if constexpr (WIDE) {
                    float4 o4;
                    o4.x = (acc[rt][T][0][r] - tt[r]) * ss[r]; o4.y = (acc[rt][T][1][r] - tt[r]) * ss[r];
                    o4.z = (acc[rt][T][2][r] - tt[r]) * ss[r]; o4.w = (acc[rt][T][3][r] - tt[r]) * ss[r];
                    *reinterpret_cast<float4*>(zb + (o0 + r) * HW + 64 * T + 4 * n) = o4;
                } else {
                    zb[(o0 + r) * HW + n] = (acc[rt][T][0][r] - tt[r]) * ss[r];
                }
            }
    }
    const float tot = cf_wave_sum(fmaf((float)HW, dsum, lsum));
    if (lane == 0) {
        const float v = tot + (lad != nullptr ? (float)HW * lad[0] : 0.f) + cadd;
        ldj[b] = accumulate ? ldj[b] + v : v;
    }
}

// h[b, c, p] = act(h[b, c, p] + bias[b, c])      (the CN(c) term of the coupling net, coupling.py:44-47)
__global__ __launch_bounds__(256) void k_add_sample_bias(float* __restrict__ h, const float* __restrict__ bias,
                                                         int HW, int64_t total, int relu) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const float v = h[e] + bias[e / HW];
        h[e] = relu ? fmaxf(v, 0.f) : v;
    }
}

// GaussianMixtureDistribution.log_prob with a context net (gaussian.py:142-158): per-sample additive shifts cm / cs
// (B, 2, M, K, D) of the component means and pre-softplus scales, constant over (h, w):
//   out[b, m] (+)= logsumexp_k [ logw[m,k] + sum_{d,p} ( -1/2 ((x - mu - cm)/sig)^2 - log sig - 1/2 log 2pi ) ],
//   sig = softplus(sG + cs).
// Work layout (forward and backward): a workgroup owns S samples (x in LDS), so every mu / sG value fetched from L2 is
// used S times; a wave owns whole channels - SEG = 2^k <= min(64, HW) lanes walk the pixels of one channel, 64/SEG
// channels side by side - so the per-channel shifts are loaded once per (component, channel) and no index division
// happens per term.  4 transcendentals per term (exp, log, rcp, log) on the hardware units: ~1e-7 relative each, far
// below the 1e-5 bits/dim tolerance after the sum over D*HW terms.
struct GmmCtxLanes {
    int SEG, CPW, G, sub, pl;
    __device__ __forceinline__ GmmCtxLanes(int D, int HW, int lane) {
        SEG = 64;
        while (SEG > HW) SEG >>= 1;                 // largest power of two <= min(64, HW)
        CPW = 64 / SEG;
        G = (D + CPW - 1) / CPW;                    // channel groups of the sample
        sub = lane / SEG;
        pl = lane - sub * SEG;
    }
};

__device__ __forceinline__ float softplus_fast(float s) { return s > 20.f ? s : __logf(1.0f + __expf(s)); }   // threshold 20, as torch

// log-joint lp[s][mk] of the S samples of this workgroup -> LDS (all threads must call; ends with a barrier)
// TAB: the scale shifts take few distinct values (embedding lookups, model.py:157,162): 1/sig and sum log sig come from
// tables indexed by the sample's key (cf_gmm_ctx_tables) - no transcendental left in the term loop.
struct GmmTab {
    const float* inv;      // (U, MK, N)  1 / softplus(sG + cs_u)
    const float* dsig;     // (U, MK, N)  softplus'(sG + cs_u)    (backward only)
    const float* lsum;     // (U, MK)     sum_e log softplus(sG + cs_u)
    const int* key;        // (B)         u of every sample
    const int* ckey;       // (B) or NULL: the mean shifts come from a table too - c is then (Um, MK, D) and ckey its row
};

template <int S, bool TAB>
__device__ __forceinline__ void gmm_ctx_logjoint(const float* __restrict__ xs, float* __restrict__ lpw, float* __restrict__ lp,
                                                 const float* __restrict__ mG, const float* __restrict__ sG,
                                                 const float* __restrict__ logw, const float* __restrict__ c, const int64_t (&co)[S],
                                                 const GmmTab& tb, const int64_t (&io)[S], int b0, int B, int MK,
                                                 int D, int HW, int lane, int wave) {
    const GmmCtxLanes L(D, HW, lane);
    const int N = D * HW;
    for (int mk = 0; mk < MK; ++mk) {
        const float* mu = mG + (int64_t)mk * N;
        const float* sg = sG + (int64_t)mk * N;
        float acc[S];
#pragma unroll
        for (int s = 0; s < S; ++s) acc[s] = 0.f;
        for (int g = wave; g < L.G; g += 4) {
            const int d = g * L.CPW + L.sub;
            if (d < D) {
                float cm[S], cs[S];
#pragma unroll
                for (int s = 0; s < S; ++s) { cm[s] = c[co[s] + mk * D + d]; cs[s] = TAB ? 0.f : c[co[s] + (MK + mk) * D + d]; }
                for (int p = L.pl; p < HW; p += L.SEG) {
                    const int e = d * HW + p;
                    if constexpr (TAB) {
                        const float m = mu[e];
#pragma unroll
                        for (int s = 0; s < S; ++s) {
                            const float r = (xs[s * N + e] - m - cm[s]) * tb.inv[io[s] + (int64_t)mk * N + e];
                            acc[s] = fmaf(-0.5f * r, r, acc[s]);
                        }
                    } else {
                        const float m = mu[e], sv = sg[e];
#pragma unroll
                        for (int s = 0; s < S; ++s) {
                            const float sig = softplus_fast(sv + cs[s]);
                            const float r = (xs[s * N + e] - m - cm[s]) * __frcp_rn(sig);
                            acc[s] += -0.5f * r * r - __logf(sig);
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const float v = cf_wave_sum(acc[s]);
            if (lane == 0) lpw[(wave * S + s) * MK + mk] = v;
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < S * MK; i += 256) {
        const int mk = i % MK;
        float v = ((lpw[i] + lpw[S * MK + i]) + (lpw[2 * S * MK + i] + lpw[3 * S * MK + i])) - 0.91893853320467274178f * (float)N +
                  logw[mk];
        if constexpr (TAB) v -= tb.lsum[(int64_t)tb.key[min(b0 + i / MK, B - 1)] * MK + mk];
        lp[i] = v;
    }
    __syncthreads();
}

// tables of GmmTab: one workgroup per (u, mk) row
__global__ __launch_bounds__(256) void k_gmm_ctx_tables(const float* __restrict__ sG, const float* __restrict__ cst,
                                                        float* __restrict__ inv, float* __restrict__ dsig,
                                                        float* __restrict__ lsum, int MK, int D, int HW) {
    __shared__ float part[4];
    const int u = blockIdx.x / MK, mk = blockIdx.x - u * MK, N = D * HW, tid = threadIdx.x;
    const float* sg = sG + (int64_t)mk * N;
    const float* cs = cst + ((int64_t)u * MK + mk) * D;
    const int64_t o = ((int64_t)u * MK + mk) * N;
    float acc = 0.f;
    for (int e = tid; e < N; e += 256) {
        const float t = sg[e] + cs[e / HW];
        const float sig = softplus_fast(t);
        inv[o + e] = __frcp_rn(sig);
        if (dsig) dsig[o + e] = t > 20.f ? 1.f : __frcp_rn(1.0f + __expf(-t));
        acc += __logf(sig);
    }
    acc = cf_wave_sum(acc);
    if ((tid & 63) == 0) part[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) lsum[(int64_t)u * MK + mk] = (part[0] + part[1]) + (part[2] + part[3]);
}

// lp_out (optional, (B, M*K)): the per-component log-joints, kept by the training forward for cf_gmm_ctx_bwd
template <int S, bool TAB>
__global__ __launch_bounds__(256) void k_gmm_ctx(const float* __restrict__ x, const float* __restrict__ mG,
                                                 const float* __restrict__ sG, const float* __restrict__ logw,
                                                 const float* __restrict__ c, float* __restrict__ out,
                                                 float* __restrict__ lp_out, int B, int M, int K, int D, int HW,
                                                 int64_t xbs, int accumulate, GmmTab tb) {
    extern __shared__ __align__(16) float lds[];
    const int N = D * HW, MK = M * K;
    float* xs = lds;                       // [S][N]
    float* lpw = xs + S * N;               // [4][S][MK] per-wave partial sums
    float* lp = lpw + 4 * S * MK;          // [S][MK]
    const int b0 = blockIdx.x * S, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t co[S], io[S];                  // offsets of the samples' shift rows in c (offsets, not pointers: see cf_step_common.h)
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const int b = min(b0 + s, B - 1);                       // ragged last workgroup: recompute the last sample
        co[s] = (TAB && tb.ckey) ? (int64_t)tb.ckey[b] * MK * D : (int64_t)b * 2 * MK * D;
        io[s] = TAB ? (int64_t)tb.key[b] * MK * N : 0;
        stage_copy(xs + s * N, x + (int64_t)b * xbs, N, tid);
    }
    __syncthreads();
    gmm_ctx_logjoint<S, TAB>(xs, lpw, lp, mG, sG, logw, c, co, tb, io, b0, B, MK, D, HW, lane, wave);
    for (int i = tid; i < S * M; i += 256) {
        const int s = i / M, m = i - s * M;
        if (b0 + s >= B) continue;
        const float* l = lp + s * MK + m * K;
        float mx = -INFINITY;
        for (int k = 0; k < K; ++k) mx = fmaxf(mx, l[k]);
        float z = 0.f;
        for (int k = 0; k < K; ++k) z += expf(l[k] - mx);
        const float v = mx + logf(z);
        if (accumulate) out[(int64_t)(b0 + s) * M + m] += v;
        else out[(int64_t)(b0 + s) * M + m] = v;
    }
    if (lp_out)
        for (int i = tid; i < S * MK; i += 256)
            if (b0 + i / MK < B) lp_out[(int64_t)b0 * MK + i] = lp[i];
}

// ConditionalGaussianDistribution.sample (gaussian.py:263-270): c = [mean | log_scale] (B, 2D) from the context
// embedding; x = mean + exp(log_scale) eps; logp[b] = sum_d (-1/2 log 2pi - log_scale - eps^2 / 2).
__global__ __launch_bounds__(64) void k_cond_gauss_sample(const float* __restrict__ c, const float* __restrict__ eps,
                                                          float* __restrict__ x, float* __restrict__ logp, int D) {
    const int b = blockIdx.x;
    float acc = 0.f;
    for (int d = threadIdx.x; d < D; d += 64) {
        const float mean = c[(int64_t)b * 2 * D + d], ls = c[(int64_t)b * 2 * D + D + d], e = eps[(int64_t)b * D + d];
        const float xv = mean + expf(ls) * e;
        x[(int64_t)b * D + d] = xv;
        const float r = xv - mean;
        acc += -0.91893853320467274178f - ls - 0.5f * expf(-2.0f * ls) * r * r;
    }
    acc = cf_wave_sum(acc);
    if (threadIdx.x == 0) logp[b] = acc;
}

// Sigmoid activation layer with its log-det (activations.py:234-238, temperature 1):
// y = sigmoid(x), ldj[b] = sum_d (-softplus(-x) - softplus(x)).
__global__ __launch_bounds__(64) void k_sigmoid_ldj(const float* __restrict__ x, float* __restrict__ y,
                                                    float* __restrict__ ldj, int D) {
    const int b = blockIdx.x;
    float acc = 0.f;
    for (int d = threadIdx.x; d < D; d += 64) {
        const float v = x[(int64_t)b * D + d];
        y[(int64_t)b * D + d] = 1.0f / (1.0f + expf(-v));
        const float a = fabsf(v);
        acc -= a + 2.0f * log1pf(expf(-a));            // softplus(v) + softplus(-v) = |v| + 2 log(1 + e^-|v|)
    }
    acc = cf_wave_sum(acc);
    if (threadIdx.x == 0) ldj[b] = acc;
}

// ---- backward of the context branches (specialist training under contextflow: the CN nets and the priors' embedding
// tables are the trainable parameters; the generalist's own parameters are frozen, model.py / coupling.py:36) ------

// dyn[] of the two backward LDS kernels, as CtxFwdLds.  NSB = C with the exp(-l_b) row of k_affine_ctx_bwd_data, 0 without;
// XPLANE: the x plane of k_conv1x1_ctx_bwd; MATRIX = false: sb alone (the lone ActNorm of k_affine_ctx_bwd_data).
struct CtxBwdLds {
    int CP, HWP;
    int nsb;      // sb[NSB] exp(-l_b), rounded up to 16 bytes
    int nWb;      // Wb[o][i], row stride CP (zero padded)
    int nxs;      // xs[C][HWP] if XPLANE
    int ngs;      // gs[C][HWP]
    __host__ __device__ CtxBwdLds(int C, int HW, int NSB, bool XPLANE, bool MATRIX = true)
        : CP((C + 7) & ~7), HWP(HW | 1), nsb((NSB + 3) & ~3), nWb(MATRIX ? C * CP : 0), nxs(MATRIX && XPLANE ? C * HWP : 0),
          ngs(MATRIX ? C * HWP : 0) {}
    __host__ __device__ int floats() const { return nsb + nWb + nxs + ngs; }
};

// Conv1x1 with a context net, backward: gx[b] = W_b^T gz[b];  G = sum_p gz[b][:,p] x[b][:,p]^T;
// gm[b][o][i] = G[o][i] (o > i) | G[i][i] exp(m_ii) + H W gld[b] (o == i) | 0 (o < i)      (d/d CN(c) output)
// One workgroup per sample; W_b (row stride CP), x and gz (row stride HWP = odd: the (o, i) products below walk rows
// with one lane per row) in LDS.
__global__ __launch_bounds__(256) void k_conv1x1_ctx_bwd(const float* __restrict__ x, const float* __restrict__ m,
                                                         const float* __restrict__ Wm, const float* __restrict__ gz,
                                                         const float* __restrict__ gld, float* __restrict__ gx,
                                                         float* __restrict__ gm, int C, int HW, int64_t xbs, int64_t gzbs) {
    extern __shared__ __align__(16) float dyn[];
    const CtxBwdLds L(C, HW, 0, true);
    const int CP = L.CP, HWP = L.HWP;
    float *Wb = dyn, *xs = Wb + L.nWb, *gs = xs + L.nxs;
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* mb = m + (int64_t)b * C * C;
    const float* xb = x + (int64_t)b * xbs;
    const float* gb = gz + (int64_t)b * gzbs;
    for (int e0 = tid; e0 < C * HW; e0 += 4 * 256) {   // batches of independent loads (padded rows: scalar stores)
        float xv[4], gv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) { const int e = min(e0 + i * 256, C * HW - 1); xv[i] = xb[e]; gv[i] = gb[e]; }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = e0 + i * 256;
            if (e < C * HW) { const int c = e / HW, p = e - c * HW; xs[c * HWP + p] = xv[i]; gs[c * HWP + p] = gv[i]; }
        }
    }
    build_wb_rowmajor<false>(Wb, mb, Wm, nullptr, C, CP, tid);
    __syncthreads();
    float* gxb = gx + (int64_t)b * C * HW;
    // gx = W_b^T gz over the input channels
    pixel8_product(Wb, gs, C, CP, HWP, HW, tid, [=](int i, int p, float acc) { gxb[(int64_t)i * HW + p] = acc; });
    float* gmb = gm + (int64_t)b * C * C;
    const float gl = gld[b] * (float)HW;
    for (int e = tid; e < C * C; e += 256) {          // lanes walk i (rows of xs: odd stride), o is shared
        const int o = e / C, i = e - o * C;
        float g = 0.f;
        if (o >= i) {
            const float* go = gs + o * HWP;
            const float* xi = xs + i * HWP;
            float g0 = 0.f, g1 = 0.f;
            int p = 0;
            for (; p + 1 < HW; p += 2) { g0 = fmaf(go[p], xi[p], g0); g1 = fmaf(go[p + 1], xi[p + 1], g1); }
            if (p < HW) g0 = fmaf(go[p], xi[p], g0);
            g = g0 + g1;
            if (o == i) g = g * expf(mb[e]) + gl;
        }
        gmb[e] = g;
    }
}

// ActNorm with a context net, backward: gx = gz exp(-l_b); gm[b] = [ -exp(-l_b) sum_p gz | -sum_p gz z + gld[b] ]
__global__ __launch_bounds__(256) void k_actnorm_ctx_bwd(const float* __restrict__ x, const float* __restrict__ m,
                                                         const float* __restrict__ t, const float* __restrict__ logs,
                                                         const float* __restrict__ gz, const float* __restrict__ gld,
                                                         float* __restrict__ gx, float* __restrict__ gm, int C, int HW,
                                                         int64_t xbs, int64_t gzbs) {
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* xb = x + (int64_t)b * xbs;
    const float* gb = gz + (int64_t)b * gzbs;
    float* gxb = gx + (int64_t)b * C * HW;
    for (int c = wave; c < C; c += 4) {               // a wave owns a channel at a time
        const ActNormCtxTerms a = actnorm_ctx_terms(m, b, t, logs, C, c);
        const float tv = a.t, s = a.s;
        float s0 = 0.f, s1 = 0.f;
        for (int p = lane; p < HW; p += 64) {
            const float g = gb[(int64_t)c * HW + p], z = (xb[(int64_t)c * HW + p] - tv) * s;
            gxb[(int64_t)c * HW + p] = g * s;
            s0 += g; s1 = fmaf(g, z, s1);
        }
        s0 = cf_wave_sum(s0); s1 = cf_wave_sum(s1);
        if (lane == 0) {
            gm[(int64_t)b * 2 * C + c] = -s * s0;
            gm[(int64_t)b * 2 * C + C + c] = gld[b] - s1;
        }
    }
}

// ---- the data-only backward of the Conv1x1 + ActNorm pair (the input gradient of log p(x | c): FlowSequential.score with a
// context).  Adjoint of cf_affine_ctx_fwd with respect to x alone:
//   gx[b] = W_b^T (gz[b] (.) exp(-l_b)),   W_b as in k_conv1x1_ctx (m1 == NULL: the identity),
//   l_b = m2[b, C:2C] [+ logs] (m2 == NULL: no scale)
// Neither log-det depends on x, so neither x, t nor gld is read, and none of the C x C / 2C parameter gradients of
// k_conv1x1_ctx_bwd / k_actnorm_ctx_bwd is formed.  USQ: gx is stored in the (C/4, 2H, 2W) layout in front of a Squeeze((2,2)).
// Any shape, any alignment: one workgroup per sample, W_b with exp(-l_b) folded into its rows (row stride CP) and gz (row
// stride HWP, odd) in LDS, as k_conv1x1_ctx_bwd without its xs plane and G products; a thread owns a pixel and 8 input channels.
template <bool USQ>
__global__ __launch_bounds__(256) void k_affine_ctx_bwd_data(const float* __restrict__ gz, const float* __restrict__ m1,
                                                             const float* __restrict__ Wm, const float* __restrict__ m2,
                                                             const float* __restrict__ logs, float* __restrict__ gx, int C,
                                                             int H, int W, int64_t gzbs) {
    extern __shared__ __align__(16) float dyn[];
    const int HW = H * W;
    const CtxBwdLds L(C, HW, C, false);
    const int CP = L.CP, HWP = L.HWP;
    float *sb = dyn, *Wb = sb + L.nsb, *gs = Wb + L.nWb;          // Wb[o][i] = W_b[o][i] exp(-l_b[o])
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* gb = gz + (int64_t)b * gzbs;
    float* gxb = gx + (int64_t)b * C * HW;
    for (int c = tid; c < C; c += 256)
        sb[c] = m2 != nullptr ? actnorm_ctx_terms<false>(m2, b, nullptr, logs, C, c).s : 1.f;
    __syncthreads();
    if (m1 == nullptr) {                              // ActNorm alone: a scale per channel
        for (int e0 = tid; e0 < C * HW; e0 += 4 * 256) {
            float gv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) gv[i] = gb[min(e0 + i * 256, C * HW - 1)];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int e = e0 + i * 256;
                if (e < C * HW) { const int c = e / HW, p = e - c * HW; gxb[USQ ? squeeze_index(c, p, W, HW) : e] = gv[i] * sb[c]; }
            }
        }
        return;
    }
    const float* mb = m1 + (int64_t)b * C * C;
    for (int e0 = tid; e0 < C * HW; e0 += 8 * 256) {   // batches of independent loads (padded rows: scalar stores)
        float gv[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) gv[i] = gb[min(e0 + i * 256, C * HW - 1)];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int e = e0 + i * 256;
            if (e < C * HW) { const int c = e / HW, p = e - c * HW; gs[c * HWP + p] = gv[i]; }
        }
    }
    build_wb_rowmajor<true>(Wb, mb, Wm, sb, C, CP, tid);
    __syncthreads();
    // gx = W_b^T (s gz) over the input channels
    pixel8_product(Wb, gs, C, CP, HWP, HW, tid, [=](int i, int p, float acc) { gxb[USQ ? squeeze_index(i, p, W, HW) : i * HW + p] = acc; });
}

// ---- the pair backwards (FlowSequential.inverse / decode / sample with a context): the inverse of cf_affine_ctx_fwd,
//   x[b] = W_b^-1 (z[b] (.) exp(l_b) + t_b) per pixel,   W_b as in k_conv1x1_ctx (m1 == NULL: the identity - a streaming pass),
//   [t_b | l_b] = m2[b] [+ t | logs] (m2 == NULL: y = z).
// It inverts the map z = W_b x the forward applies: under contextflow W_b is a full matrix (whatever log-det the forward reports).
// dyn[] of the kernel, as CtxFwdLds: MATRIX = false is the lone ActNorm.
struct CtxInvLds {
    int CP, S;
    int nAt;      // At[k][c] = W_b^-1[c][k], row stride CP (zero padded): the operand of pixel8_product
    int nys;      // ys[C][HW] = z exp(l_b) + t_b
    int nxs;      // xs[C][HW]: the first solution x0 = W_b^-1 y, kept for the refinement step
    int nA;       // A[C][S]: W_b, inverted in place, then W_b again; S = C + 1 (the column walks of the elimination meet no bank twice)
    int nc;       // tb[C] = t_b, eb[C] = exp(l_b), colk[C], rowk[C], rowo[C], piv[C] (int), rounded up to 4 floats each
    __host__ __device__ CtxInvLds(int C, int HW, bool MATRIX)
        : CP((C + 7) & ~7), S(C + 1), nAt(MATRIX ? C * CP : 0), nys(MATRIX ? C * HW : 0), nxs(nys), nA(MATRIX ? C * (C + 1) : 0),
          nc((C + 3) & ~3) {}
    __host__ __device__ int floats() const { return nAt + nys + nxs + nA + (nA ? 6 : 2) * nc; }
};

// One workgroup per sample.  W_b (build_wb_rowmajor: the LDS family's rounding) is inverted in place by fp32 Gauss-Jordan with
// partial (row) pivoting - the arithmetic of k_inverse_lds (cf_linalg.hip): per pivot a search, a row swap, the scaled pivot row and
// one rank-1 update of the C x C block; the column swaps that undo the row pivoting run at the end - and its transpose
// multiplies the staged y.  Every loop is bounded by C: a zero pivot gives a non-finite x, never a hang.  C^3 / 256 FMAs per thread
// for the inverse next to C^2 HW / 256 for the product.
// One step of iterative refinement follows: x = x0 + W_b^-1 (y - W_b x0) with the residual accumulated in fp64.  An fp32 inverse
// times y errs by cond(W_b) eps - 1e-4 of scale at the condition numbers of 1e3 .. 1e4 that trained contextflow layers reach, and
// up to 20 x what an fp32 LU solve loses on the lower triangular W_b without contextflow - and the chain multiplies such steps;
// the refined x is within eps + (cond eps)^2 of the exact one.  It costs two more products over data that is in LDS already.
// TR (cf_affine_ctx_inv_bwd_data): the vector-Jacobian product of that map, which is affine in z:  gz[b] = e^{l_b} (.) (W_b^-T gx[b]).
// `z` is gx, `x` receives gz, t is not read.  The same W_b is inverted by the same elimination - the inverse of the transpose is the
// transpose of the inverse - and only the READS change: the product takes A = W_b^-1 row by row where the plain form takes its
// transpose, the fp64 residual gx - W_b^T g0 walks W_b by columns; the scale moves from the load to the store, there is no shift.
// USQ then says that gx ARRIVES in the (C/4, 2H, 2W) layout (the walk's output): the index map folds into the staging loads.
template <bool USQ, bool TR = false>
__global__ __launch_bounds__(256) void k_affine_ctx_inv(const float* __restrict__ z, const float* __restrict__ m1,
                                                        const float* __restrict__ Wm, const float* __restrict__ m2,
                                                        const float* __restrict__ t, const float* __restrict__ logs,
                                                        float* __restrict__ x, int C, int H, int W, int64_t zbs) {
    extern __shared__ __align__(16) float dyn[];
    const int HW = H * W;
    const CtxInvLds L(C, HW, m1 != nullptr);
    const int CP = L.CP, S = L.S;
    float *At = dyn, *ys = At + L.nAt, *xs = ys + L.nys, *A = xs + L.nxs, *tb = A + L.nA, *eb = tb + L.nc;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const float* zb = z + (int64_t)b * zbs;
    float* xb = x + (int64_t)b * C * HW;
    for (int c = tid; c < C; c += 256) {
        float tv = 0.f, ev = 1.f;
        if (m2 != nullptr) {
            if constexpr (TR) {
                ev = expf(actnorm_ctx_terms<false>(m2, b, nullptr, logs, C, c).l);
            } else {
            const ActNormCtxTerms a = actnorm_ctx_terms(m2, b, t, logs, C, c);
            tv = a.t; ev = expf(a.l);
            }
        }
        tb[c] = tv; eb[c] = ev;
    }
    __syncthreads();
    if (m1 == nullptr) {                              // ActNorm alone: a scale and a shift per channel
        for (int e0 = tid; e0 < C * HW; e0 += 4 * 256) {
            float zv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int e = min(e0 + i * 256, C * HW - 1);
                zv[i] = zb[(TR && USQ) ? squeeze_index(e / HW, e % HW, W, HW) : e];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int e = e0 + i * 256;
                if (e < C * HW) {
                    const int c = e / HW, p = e - c * HW;
                    if constexpr (TR) xb[e] = zv[i] * eb[c];
                    else xb[USQ ? squeeze_index(c, p, W, HW) : e] = fmaf(zv[i], eb[c], tb[c]);
                }
            }
        }
        return;
    }
    float* colk = eb + L.nc;                           // per pivot: column k of the matrix as it was (0 at the pivot row)
    float* rowk = colk + L.nc;                         // ... the new pivot row: row p / pivot, 1 / pivot at column k
    float* rowo = rowk + L.nc;                         // ... the old row k (column k zeroed): it moves to row p
    int* piv = reinterpret_cast<int*>(rowo + L.nc);
    // y = z exp(l_b) + t_b -> LDS (batches of independent loads, in flight while the matrix is built)
    for (int e0 = tid; e0 < C * HW; e0 += 8 * 256) {
        float zv[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int e = min(e0 + i * 256, C * HW - 1);
            zv[i] = zb[(TR && USQ) ? squeeze_index(e / HW, e % HW, W, HW) : e];
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int e = e0 + i * 256;
            if (e < C * HW) { const int c = e / HW; ys[e] = TR ? zv[i] : fmaf(zv[i], eb[c], tb[c]); }
        }
    }
    build_wb_rowmajor<false>(A, m1 + (int64_t)b * C * C, Wm, nullptr, C, S, tid);
    __syncthreads();
    // this thread's walk over the C x C block in steps of 256 elements: (row, column) of its first element and the step
    const int r0 = tid / C, c0 = tid - r0 * C, dr = 256 / C, dc = 256 - dr * C;
    // The elimination is bound by the vector instructions it issues (C^3 / 256 element updates per thread), so a thread owns ONE
    // column c0 and the block of rows [ra, rb) - row group r0 of the 256 / C groups - and an update is a read, a select, an FMA
    // and a write at addresses one row stride apart.  Two barriers per pivot: every wave finds the pivot row for itself, what the
    // rank-1 update reads of the old matrix is staged - its column k and the rows k and p, the swap folded in - and every element
    // is then updated from the staged vectors alone; the rows k and p are put right by their owners behind the sweep.
    const int RG = (C + dr - 1) / dr, ra = min(r0 * RG, C), rb = r0 < dr ? min(ra + RG, C) : ra;
    for (int k = 0; k < C; ++k) {
        // pivot search over rows k .. C-1 of column k: key = (bits of |a|, ~row), so the maximum is the largest |a| at the lowest row
        unsigned long long key = 0ull;
        for (int r = k + lane; r < C; r += 64) {
            const unsigned long long kv = ((unsigned long long)__float_as_uint(fabsf(A[r * S + k])) << 32) | (0xFFFFFFFFu - (unsigned)r);
            key = kv > key ? kv : key;
        }
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long ok = __shfl_xor(key, o, 64);
            key = ok > key ? ok : key;
        }
        const int p = (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull));
        if (tid == 0) piv[k] = p;
        const float d = 1.0f / A[p * S + k], akk = A[k * S + k];
        for (int c = tid; c < C; c += 256) {
            const float ap = A[p * S + c], ak = A[k * S + c], ac = A[c * S + k];
            rowk[c] = (c == k ? 1.0f : ap) * d;
            rowo[c] = c == k ? 0.f : ak;
            colk[c] = (c == k || c == p) ? 0.f : ac;            // (rows k and p: written behind the sweep)
        }
        __syncthreads();
        const float rk = rowk[c0];
        const bool zc = c0 == k;
        float* col = A + c0;
        for (int r = ra; r < rb; r += 8) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = col[min(r + j, rb - 1) * S];
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (r + j < rb) col[(r + j) * S] = fmaf(-colk[r + j], rk, zc ? 0.f : v[j]);
        }
        if (p != k && p >= ra && p < rb) col[p * S] = fmaf(-akk, rk, rowo[c0]);
        if (k >= ra && k < rb) col[k * S] = rk;
        __syncthreads();
    }
    for (int k = C - 1; k >= 0; --k) {
        const int p = piv[k];                         // (the same for every thread: the barrier is uniform)
        if (p != k) {
            for (int r = tid; r < C; r += 256) { const float v = A[r * S + k]; A[r * S + k] = A[r * S + p]; A[r * S + p] = v; }
            __syncthreads();
        }
    }
    // At[k][c] = W_b^-1[c][k]: lanes walk c (A at stride S, At contiguous), padding columns zero
    for (int kk = r0, c = c0; kk < C;) {
        At[kk * CP + c] = TR ? A[kk * S + c] : A[c * S + kk];             // (TR: W_b^-T[c][k], a straight copy)
        kk += dr; c += dc;
        if (c >= C) { c -= C; ++kk; }
    }
    for (int e = tid; e < C * (CP - C); e += 256) { const int kk = e / (CP - C); At[kk * CP + C + (e - kk * (CP - C))] = 0.f; }
    __syncthreads();
    build_wb_rowmajor<false>(A, m1 + (int64_t)b * C * C, Wm, nullptr, C, S, tid);          // W_b again, for the residual
    pixel8_product(At, ys, C, CP, HW, HW, tid, [=](int c, int p, float acc) { xs[c * HW + p] = acc; });
    __syncthreads();
    // ys <- y - W_b x0 in fp64: a thread owns a pixel and 8 rows of W_b (TR: columns, W_b^T), and is the only reader of the y it replaces
    for (int e = tid; e < (CP >> 3) * HW; e += 256) {
        const int cb = e / HW, p = e - cb * HW, c0 = cb * 8;
        double acc[8];
        int row[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) { row[k] = min(c0 + k, C - 1) * (TR ? 1 : S); acc[k] = (double)ys[min(c0 + k, C - 1) * HW + p]; }
        for (int i = 0; i < C; ++i) {
            const double xv = (double)xs[i * HW + p];
#pragma unroll
            for (int k = 0; k < 8; ++k) acc[k] = fma(-(double)(TR ? A[i * S + row[k]] : A[row[k] + i]), xv, acc[k]);
        }
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (c0 + k < C) ys[(c0 + k) * HW + p] = (float)acc[k];
    }
    __syncthreads();
    pixel8_product(At, ys, C, CP, HW, HW, tid,
                   [=](int c, int p, float acc) {
                       if constexpr (TR) xb[c * HW + p] = eb[c] * (xs[c * HW + p] + acc);
                       else xb[USQ ? squeeze_index(c, p, W, HW) : c * HW + p] = xs[c * HW + p] + acc;
                   });
}

// The three levels of the image flows: k_affine_ctx_wave transposed - one wave per sample, no LDS, no barrier, 64
// v_mfma_f32_16x16x4_f32 per sample, every operand read from global memory once.
//   A (W_b^T with exp(-l_b) folded into its columns; 16 rows i x 4 k = o per instruction): lane (n, kk) holds
//     W_b[o = 16 g + 4 kk + e][i = 16 it + n] exp(-l_b[o]), e = 0..3, for four successive k-steps - a column walk of the row-major
//     m1 (dwords, 64-byte runs over n); blocks g < it hold NN alone.  The scale costs C^2 / 64 multiplies per lane, not C HW.
//   B (gz): for those k-steps lane (n, kk) needs gz[o = 16 g + 4 kk + e][pixel of column n] - exactly the forward's x loads.
//   D: lane (n, kk) holds rows i = 16 it + 4 kk + r: float4 stores over the four column tiles; USQ: the four rows are the four
//     phases of ONE channel q = 4 it + kk of the un-squeezed tensor (the mirror of the forward's SQ loads).
// The k-step loop runs over the row tiles / column tiles innermost: successive MFMAs never share an accumulator (the fp32
// 16x16x4 form issues every 32 cycles and returns after 40).
template <int C, int W, bool USQ>
__global__ __launch_bounds__(256) void k_affine_ctx_bwd_wave(const float* __restrict__ gz, const float* __restrict__ m1,
                                                             const float* __restrict__ Wm, const float* __restrict__ m2,
                                                             const float* __restrict__ logs, float* __restrict__ gx, int B,
                                                             int64_t gzbs) {
    using G = AffineWave<C, W>;
    constexpr int HW = G::HW, RT = G::RT, NG = G::NG, WIDE = G::WIDE, NT = G::NT, NJ = G::NJ;
    const int lane = threadIdx.x & 63, n = lane & 15, kk = lane >> 4;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;                                // a whole wave: the kernel has no barrier
    const float* mb = m1 + (int64_t)b * C * C;
    const float* gb = gz + (int64_t)b * gzbs;
    float4 a[RT][NG];
    float dsum = 0.f;                                  // (the diagonal sum wb_element_wave keeps: not used here)
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const int o0 = 16 * g + 4 * kk;
        float ss[4] = {1.f, 1.f, 1.f, 1.f};
        if (m2 != nullptr) {
            float4 tv, lv;                             // (tv: not formed)
            G::template actnorm_rows<false>(m2, b, nullptr, logs, o0, tv, lv);
            ss[0] = expf(-lv.x); ss[1] = expf(-lv.y); ss[2] = expf(-lv.z); ss[3] = expf(-lv.w);
        }
#pragma unroll
        for (int it = 0; it < RT; ++it) {
            const int i = 16 * it + n;
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = g >= it ? mb[(o0 + e) * C + i] : 0.f;
            if (g == it) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = wb_element_wave(v[e], Wm != nullptr, o0 + e, i, dsum);
            }
            if (Wm != nullptr) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] += Wm[(o0 + e) * C + i];
            }
            a[it][g] = make_float4(v[0] * ss[0], v[1] * ss[1], v[2] * ss[2], v[3] * ss[3]);
        }
    }
    float* gxb = gx + (int64_t)b * C * HW;
#pragma unroll
    for (int T = 0; T < NT; ++T) {
        f32x4 acc[RT][NJ];
#pragma unroll
        for (int it = 0; it < RT; ++it)
#pragma unroll
            for (int j = 0; j < NJ; ++j) acc[it][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            float gv[4][NJ];                           // [k-step e][column tile j]
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if constexpr (WIDE) {
                    const float4 v = *reinterpret_cast<const float4*>(gb + (16 * g + 4 * kk + e) * HW + 64 * T + 4 * n);
                    gv[e][0] = v.x; gv[e][1] = v.y; gv[e][2] = v.z; gv[e][3] = v.w;
                } else {
                    gv[e][0] = gb[(16 * g + 4 * kk + e) * HW + n];
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int it = 0; it < RT; ++it) {
                    const float av = e == 0 ? a[it][g].x : (e == 1 ? a[it][g].y : (e == 2 ? a[it][g].z : a[it][g].w));
#pragma unroll
                    for (int j = 0; j < NJ; ++j) acc[it][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, gv[e][j], acc[it][j], 0, 0, 0);
                }
        }
#pragma unroll
        for (int it = 0; it < RT; ++it) {
            if constexpr (!USQ) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = 16 * it + 4 * kk + r;
                    if constexpr (WIDE)
                        *reinterpret_cast<float4*>(gxb + i * HW + 64 * T + 4 * n) =
                            make_float4(acc[it][0][r], acc[it][1][r], acc[it][2][r], acc[it][3][r]);
                    else
                        gxb[i * HW + n] = acc[it][0][r];
                }
            } else {
                const int p0 = G::pixel0(T, n), yy = p0 / W, xx = p0 - yy * W;
#pragma unroll
                for (int dy = 0; dy < 2; ++dy) {                // rows r = 2 dy + dx: the phases of channel q = 4 it + kk
                    float* row = G::phase_row(gxb, 4 * it + kk, dy, yy, xx);
                    if constexpr (WIDE) {
                        *reinterpret_cast<float4*>(row) =
                            make_float4(acc[it][0][2 * dy], acc[it][0][2 * dy + 1], acc[it][1][2 * dy], acc[it][1][2 * dy + 1]);
                        *reinterpret_cast<float4*>(row + 4) =
                            make_float4(acc[it][2][2 * dy], acc[it][2][2 * dy + 1], acc[it][3][2 * dy], acc[it][3][2 * dy + 1]);
                    } else {
                        *reinterpret_cast<float2*>(row) = make_float2(acc[it][0][2 * dy], acc[it][0][2 * dy + 1]);
                    }
                }
            }
        }
    }
}

// out[b, c] = sum_p a[b, c, p]      (d/d of a per-sample bias: row sums of a gradient plane)
__global__ __launch_bounds__(256) void k_sample_channel_sums(const float* __restrict__ a, float* __restrict__ out, int HW,
                                                             int64_t rows) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    float s = 0.f;
    for (int p = lane; p < HW; p += 64) s += a[row * HW + p];
    s = cf_wave_sum(s);
    if (lane == 0) out[row] = s;
}

// y = gy * (x > 0)   (ReLU backward of the CN nets)
__global__ __launch_bounds__(256) void k_relu_bwd(const float* __restrict__ x, const float* __restrict__ gy,
                                                  float* __restrict__ out, int64_t n) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256)
        out[e] = x[e] > 0.f ? gy[e] : 0.f;
}

// GMM with a context net, backward w.r.t. x and the per-sample shifts (gaussian.py:142-158; parameters frozen):
// r[mk] = g[b,m] softmax_k(lp)[mk];  with d = x - mu - cm, sig = softplus(s), s = sG + cs:
//   gx[e]      = sum_mk r * (-d / sig^2)
//   gc[0][mk][dch] = sum_hw r * d / sig^2
//   gc[1][mk][dch] = sum_hw r * (d^2 / sig^3 - 1 / sig) * sigmoid(s)
// Same work layout as k_gmm_ctx: S samples per workgroup, a wave owns channels.  With the channel fixed and the
// component loop inside, gx accumulates in registers (PIT pixels per lane and sample) and the (component, channel)
// sums are segmented shuffle reductions over the SEG lanes of the channel.  lp_in (optional): the log-joints kept by
// the forward; without it they are recomputed first.
// DATA = true (cf_gmm_ctx_bwd_data: the input gradient alone, FlowSequential.score with a context): no dsig reads, no a0 / a1
// sums, no segmented reductions and no gc stores (gc may be null); the gx accumulation is the same instruction stream, so gx is
// bit for bit the training form's.
template <int S, bool TAB, bool DATA = false>
__global__ __launch_bounds__(256) void k_gmm_ctx_bwd(const float* __restrict__ x, const float* __restrict__ mG,
                                                     const float* __restrict__ sG, const float* __restrict__ logw,
                                                     const float* __restrict__ c, const float* __restrict__ g,
                                                     const float* __restrict__ lp_in, float* __restrict__ gx,
                                                     float* __restrict__ gc, int B, int M, int K, int D, int HW,
                                                     int64_t xbs, GmmTab tb) {
    constexpr int PIT = 4;                 // pixels per lane and pass
    extern __shared__ __align__(16) float lds[];
    const int N = D * HW, MK = M * K;
    float* xs = lds;                       // [S][N]
    float* lpw = xs + S * N;               // [4][S][MK]
    float* lp = lpw + 4 * S * MK;          // [S][MK] log-joint, then responsibilities x upstream gradient
    const int b0 = blockIdx.x * S, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t co[S], io[S];
    bool live[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const int b = min(b0 + s, B - 1);
        live[s] = b0 + s < B;
        co[s] = (int64_t)b * 2 * MK * D;
        io[s] = TAB ? (int64_t)tb.key[b] * MK * N : 0;
        stage_copy(xs + s * N, x + (int64_t)b * xbs, N, tid);
    }
    __syncthreads();
    if (lp_in) {
        for (int i = tid; i < S * MK; i += 256) lp[i] = lp_in[(int64_t)min(b0 + i / MK, B - 1) * MK + i % MK];
        __syncthreads();
    } else {
        gmm_ctx_logjoint<S, TAB>(xs, lpw, lp, mG, sG, logw, c, co, tb, io, b0, B, MK, D, HW, lane, wave);
    }
    float* rr = lpw;                       // [S][MK] responsibilities (lpw is free now)
    for (int i = tid; i < S * M; i += 256) {
        const int s = i / M, m = i - s * M;
        const float* l = lp + s * MK + m * K;
        float mx = -INFINITY;
        for (int k = 0; k < K; ++k) mx = fmaxf(mx, l[k]);
        float z = 0.f;
        for (int k = 0; k < K; ++k) z += expf(l[k] - mx);
        const float gm = g[(int64_t)min(b0 + s, B - 1) * M + m] / z;
        for (int k = 0; k < K; ++k) rr[s * MK + m * K + k] = expf(l[k] - mx) * gm;
    }
    __syncthreads();
    const GmmCtxLanes L(D, HW, lane);
    for (int gi = wave; gi < L.G; gi += 4) {
        const int d = gi * L.CPW + L.sub;
        const bool dok = d < D;
        for (int p0 = 0; p0 < HW; p0 += PIT * L.SEG) {          // one pass unless HW > 4 SEG
            float gxa[S][PIT];
#pragma unroll
            for (int s = 0; s < S; ++s)
#pragma unroll
                for (int it = 0; it < PIT; ++it) gxa[s][it] = 0.f;
            for (int mk = 0; mk < MK; ++mk) {
                const float* mu = mG + (int64_t)mk * N;
                const float* sg = sG + (int64_t)mk * N;
                float cm[S], cs[S], a0[S], a1[S], r[S];
#pragma unroll
                for (int s = 0; s < S; ++s) {
                    r[s] = rr[s * MK + mk];
                    cm[s] = dok ? c[co[s] + mk * D + d] : 0.f;
                    cs[s] = (dok && !(TAB && DATA)) ? c[co[s] + (MK + mk) * D + d] : 0.f;
                    a0[s] = 0.f;
                    a1[s] = 0.f;
                }
#pragma unroll
                for (int it = 0; it < PIT; ++it) {
                    const int p = p0 + it * L.SEG + L.pl;
                    if (dok && p < HW) {
                        const int e = d * HW + p;
                        const float m = mu[e];
                        float sv = 0.f;
                        if constexpr (!TAB) sv = sg[e];
#pragma unroll
                        for (int s = 0; s < S; ++s) {
                            float inv, dsig = 0.f;
                            if constexpr (TAB) {
                                inv = tb.inv[io[s] + (int64_t)mk * N + e];
                                if constexpr (!DATA) dsig = tb.dsig[io[s] + (int64_t)mk * N + e];
                            } else {
                                const float t = sv + cs[s];
                                inv = __frcp_rn(softplus_fast(t));
                                if constexpr (!DATA) dsig = t > 20.f ? 1.f : __frcp_rn(1.0f + __expf(-t));   // softplus'
                            }
                            const float dd = xs[s * N + e] - m - cm[s];
                            const float q = dd * inv * inv;                                  // d / sig^2
                            gxa[s][it] = fmaf(-r[s], q, gxa[s][it]);
                            if constexpr (!DATA) {
                                a0[s] += q;
                                a1[s] += (dd * q * inv - inv) * dsig;
                            }
                        }
                    }
                }
                if constexpr (!DATA) {
#pragma unroll
                    for (int s = 0; s < S; ++s) {
                        for (int o = L.SEG >> 1; o > 0; o >>= 1) { a0[s] += __shfl_xor(a0[s], o, 64); a1[s] += __shfl_xor(a1[s], o, 64); }
                        if (L.pl == 0 && dok && live[s]) {
                            float* gcb = gc + co[s];
                            if (p0 == 0) { gcb[mk * D + d] = r[s] * a0[s]; gcb[(MK + mk) * D + d] = r[s] * a1[s]; }
                            else { gcb[mk * D + d] += r[s] * a0[s]; gcb[(MK + mk) * D + d] += r[s] * a1[s]; }
                        }
                    }
                }
            }
#pragma unroll
            for (int s = 0; s < S; ++s)
#pragma unroll
                for (int it = 0; it < PIT; ++it) {
                    const int p = p0 + it * L.SEG + L.pl;
                    if (dok && p < HW && live[s]) gx[(int64_t)(b0 + s) * N + d * HW + p] = gxa[s][it];
                }
        }
    }
}

// h[b, c2, p] += x[b, c2 % C, p]   (the identity branch of MaskedResidualBlock2d: x repeated along channels,
// autoregressive/masked_conv_2d.py:93-98)
__global__ __launch_bounds__(256) void k_add_repeat(float* __restrict__ h, const float* __restrict__ x, int C2, int C,
                                                    int HW, int64_t total) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t b = e / ((int64_t)C2 * HW);
        const int r = (int)(e - b * (int64_t)C2 * HW), c2 = r / HW, p = r - c2 * HW;
        h[e] += x[(b * C + (c2 % C)) * HW + p];
    }
}

// Gradient w.r.t. the prior's OWN parameters for specialists trained without contextflow (gaussian.py:130-137: mG / sG / wG
// stay trainable), table form of the scale shifts:
//   gm[mk][e] = sum_b r[b][mk] d / sig^2,   gs[mk][e] = sum_b r[b][mk] (d^2 / sig^3 - 1 / sig) softplus'(s)
// with d = x - mu - cm, r = upstream gradient x responsibility.  A thread owns one (mk, e) and walks a slab of SB
// samples; the per-slab partials (nb, MK, N) are summed by the caller in slab order.
__global__ __launch_bounds__(256) void k_gmm_ctx_pgrad(const float* __restrict__ x, const float* __restrict__ mG,
                                                       const float* __restrict__ c, const float* __restrict__ r,
                                                       float* __restrict__ pgm, float* __restrict__ pgs, int B, int MK,
                                                       int D, int HW, int64_t xbs, int SB, GmmTab tb) {
    const int N = D * HW, e = blockIdx.x * 256 + threadIdx.x, mk = blockIdx.y;
    if (e >= N) return;
    const int d = e / HW, b0 = blockIdx.z * SB, b1 = min(B, b0 + SB);
    const float mu = mG[(int64_t)mk * N + e];
    float am = 0.f, as = 0.f;
    for (int b = b0; b < b1; ++b) {
        const int64_t o = ((int64_t)tb.key[b] * MK + mk) * N + e;
        const float rb = r[(int64_t)b * MK + mk];
        const float iv = tb.inv[o], ds = tb.dsig[o];
        const float dd = x[(int64_t)b * xbs + e] - mu - c[(int64_t)b * 2 * MK * D + mk * D + d];
        const float q = dd * iv * iv;
        am = fmaf(rb, q, am);
        as = fmaf(rb, (dd * q * iv - iv) * ds, as);
    }
    const int64_t po = ((int64_t)blockIdx.z * MK + mk) * N + e;
    pgm[po] = am;
    pgs[po] = as;
}

// samples per workgroup of the context-GMM kernels: as many as fit (x of S samples + the log-joint scratch in LDS)
static int gmm_ctx_group(int N, int MK, size_t* lds) {
    for (int S = 4; S >= 1; S >>= 1) {
        *lds = (size_t)(S * N + 5 * S * MK) * sizeof(float);
        if (*lds <= 64 * 1024) return S;
    }
    return *lds <= 160 * 1024 ? 1 : 0;
}

// The launch of a context-GMM kernel family K<S> (a generic functor: K(std::integral_constant<int, S>) is the kernel for S
// samples per workgroup): S as gmm_ctx_group says, K<1> alone can need more than 64 KiB.
template <class K, class... A>
static int gmm_ctx_launch(const char* who, const char* func, std::atomic<uint64_t>& raised, K kernel, int B, int D, int HW, int MK,
                          hipStream_t st, A... args) {
    size_t lds;
    const int S = gmm_ctx_group(D * HW, MK, &lds);
    if (S == 0) { cf_set_error("%s: D*HW=%d needs %zu B of LDS", who, D * HW, lds); return CF_ERR_UNSUPPORTED; }
    if (lds > 64 * 1024)
        if (int rc_ = cf_raise_dynamic_lds((const void*)kernel(std::integral_constant<int, 1>{}), 160 * 1024, raised, func)) return rc_;
    const dim3 grid((B + S - 1) / S);
    if (S == 4) kernel(std::integral_constant<int, 4>{})<<<grid, dim3(256), lds, st>>>(args...);
    else if (S == 2) kernel(std::integral_constant<int, 2>{})<<<grid, dim3(256), lds, st>>>(args...);
    else kernel(std::integral_constant<int, 1>{})<<<grid, dim3(256), lds, st>>>(args...);
    return 0;
}

template <bool TAB>
static int gmm_ctx_fwd_launch(const char* who, const float* x, const float* mG, const float* sG, const float* logw, const float* c,
                              float* out, float* lp_out, int B, int M, int K, int D, int HW, int64_t xbs, int accumulate,
                              GmmTab tb, hipStream_t st) {
    static std::atomic<uint64_t> raised{0};
    return gmm_ctx_launch(who, __func__, raised, [](auto s) { return k_gmm_ctx<decltype(s)::value, TAB>; }, B, D, HW, M * K, st,
                          x, mG, sG, logw, c, out, lp_out, B, M, K, D, HW, xbs, accumulate, tb);
}

template <bool TAB, bool DATA = false>
static int gmm_ctx_bwd_launch(const char* who, const float* x, const float* mG, const float* sG, const float* logw, const float* c,
                              const float* g, const float* lp, float* gx, float* gc, int B, int M, int K, int D, int HW,
                              int64_t xbs, GmmTab tb, hipStream_t st) {
    static std::atomic<uint64_t> raised{0};
    return gmm_ctx_launch(who, __func__, raised, [](auto s) { return k_gmm_ctx_bwd<decltype(s)::value, TAB, DATA>; }, B, D, HW, M * K, st,
                          x, mG, sG, logw, c, g, lp, gx, gc, B, M, K, D, HW, xbs, tb);
}

// ---- host side of the Conv1x1 / ActNorm kernels

// the three levels of the image flows, which k_affine_ctx_wave / k_affine_ctx_bwd_wave are instantiated for
static bool affine_wave_shape(int C, int H, int W) {
    return H == W && ((C == 16 && W == 16) || (C == 32 && W == 8) || (C == 64 && W == 4));
}

// every pointer 16-byte aligned (NULL counts as aligned)
template <class... P>
static bool aligned16(const P*... p) { return ((... | reinterpret_cast<uintptr_t>(p)) & 15) == 0; }

// One workgroup of 256 threads per sample with `floats` of dynamic LDS, for the per-sample LDS kernels: refused above the
// 160 KiB of a CU, the limit of the kernel raised above 64 KiB (once per kernel and device: `raised` is per instantiation).
template <auto Kernel, class... A>
static int launch_per_sample(const char* who, int B, int C, int HW, int floats, hipStream_t st, A... args) {
    const size_t lds = (size_t)floats * sizeof(float);
    if (lds > 160 * 1024) { cf_set_error("%s: C=%d, H*W=%d need %zu B of LDS", who, C, HW, lds); return CF_ERR_UNSUPPORTED; }
    if (lds > 64 * 1024) {
        static std::atomic<uint64_t> raised{0};
        if (int rc_ = cf_raise_dynamic_lds((const void*)Kernel, 160 * 1024, raised, who)) return rc_;
    }
    Kernel<<<dim3(B), dim3(256), lds, st>>>(args...);
    return 0;
}

// grid of the grid-stride elementwise kernels (256 threads) over n elements
static dim3 grid_stride_blocks(int64_t n) { return dim3((unsigned)std::min<int64_t>((n + 255) / 256, 16384)); }

}  // namespace

extern "C" {

int cf_ctx_encode(const int64_t* ctx, const float* u, const float* qbins, const int64_t* card, float* out, int B, int nctx,
                  int width, int onehot, cf_stream_t stream) {
    if (B == 0) return 0;
    CF_REQUIRE(ctx && u && out && B >= 0 && nctx > 0 && width > 0 && (!onehot || card) && (onehot == 2 || qbins));
    const int64_t total = (int64_t)B * width;
    k_ctx_encode<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, cf_s(stream)>>>(ctx, u, qbins, card, out, B, nctx,
                                                                                       width, onehot);
    CF_LAUNCH_CHECK();
    return 0;
}

int cf_conv1x1_ctx(const float* x, const float* m, const float* Wm, float* z, float* ldj, int B, int C, int HW,
                   int64_t x_bstride, cf_stream_t stream) {
    if (B == 0) return 0;
    CF_REQUIRE(x && m && z && ldj && B >= 0 && C > 0 && HW > 0);
    if (int rc = launch_per_sample<k_conv1x1_ctx>(__func__, B, C, HW, CtxFwdLds(C, HW, 0).floats(), cf_s(stream), x, m, Wm, z, ldj, C, HW,
                                                  x_bstride)) return rc;
    CF_LAUNCH_CHECK();
    return 0;
}

// number of floats per sample of the blocked form of m1 (cf_affine_ctx_fwd, m1_blocked != 0), 0 where it is not offered
int cf_affine_ctx_blocked_floats(int C, int H, int W) {
    return affine_wave_shape(C, H, W) ? (C / 16) * (C / 16 + 1) / 2 * 256 : 0;
}

int cf_affine_ctx_fwd(const float* x, const float* m1, const float* Wm, const float* m2, const float* t, const float* logs,
                      const float* lad, float cadd, float* z, float* ldj, int B, int C, int H, int W, int64_t x_bstride,
                      int in_squeeze, int accumulate, int m1_blocked, cf_stream_t stream) {
    if (B == 0) return 0;
    CF_REQUIRE(!m1_blocked || cf_affine_ctx_blocked_floats(C, H, W) > 0);
    CF_REQUIRE(x && m1 && m2 && z && ldj && B >= 0 && C > 0 && C <= 256 && H > 0 && W > 0 && ((t == nullptr) == (logs == nullptr)) &&
               x_bstride >= (int64_t)C * H * W && (!in_squeeze || C % 4 == 0));
    // the image flows' three levels: one wave per sample on the matrix pipe, operands straight from global memory
    if (affine_wave_shape(C, H, W) && aligned16(x, m1, m2, z, Wm, t, logs) && x_bstride % 4 == 0) {
        const dim3 grid((B + 3) / 4), blk(256);
#define CF_AFF2(CC, WW, SQV, BLV) k_affine_ctx_wave<CC, WW, SQV, BLV><<<grid, blk, 0, cf_s(stream)>>>(x, m1, Wm, m2, t, logs, lad, cadd, z, ldj, B, x_bstride, accumulate)
#define CF_AFF(CC, WW) do { if (in_squeeze) { if (m1_blocked) CF_AFF2(CC, WW, true, true); else CF_AFF2(CC, WW, true, false); } \
                            else { if (m1_blocked) CF_AFF2(CC, WW, false, true); else CF_AFF2(CC, WW, false, false); } } while (0)
        if (C == 16) CF_AFF(16, 16); else if (C == 32) CF_AFF(32, 8); else CF_AFF(64, 4);
#undef CF_AFF
#undef CF_AFF2
        CF_LAUNCH_CHECK();
        return 0;
    }
    CF_REQUIRE(!m1_blocked);                             // (the blocked form exists for the wave kernel's shapes and needs their alignment)
    const int floats = CtxFwdLds(C, H * W, C).floats();
    if (int rc = in_squeeze ? launch_per_sample<k_affine_ctx<true>>(__func__, B, C, H * W, floats, cf_s(stream), x, m1, Wm, m2, t, logs, lad,
                                                                    cadd, z, ldj, C, H, W, x_bstride, accumulate)
                            : launch_per_sample<k_affine_ctx<false>>(__func__, B, C, H * W, floats, cf_s(stream), x, m1, Wm, m2, t, logs, lad,
                                                                     cadd, z, ldj, C, H, W, x_bstride, accumulate)) return rc;
    CF_LAUNCH_CHECK();
    return 0;
}

int cf_actnorm_ctx(const float* x, const float* m, const float* t, const float* logs, float* z, float* ldj, int B, int C,
                   int HW, int64_t x_bstride, cf_stream_t stream) {
    if (B == 0) return 0;
    CF_REQUIRE(x && m && z && ldj && B >= 0 && C > 0 && HW > 0 && ((t == nullptr) == (logs == nullptr)));
    if (C > 128) { cf_set_error("cf_actnorm_ctx: C=%d > 128 unsupported", C); return CF_ERR_UNSUPPORTED; }
    k_actnorm_ctx<<<dim3(B), dim3(256), 0, cf_s(stream)>>>(x, m, t, logs, z, ldj, C, HW, x_bstride);
    CF_LAUNCH_CHECK();
    return 0;
}

int cf_add_sample_bias(float* h, const float* bias, int B, int C, int HW, int relu, cf_stream_t stream) {
    if (B == 0) return 0;
    CF_REQUIRE(h && bias && B >= 0 && C > 0 && HW > 0);
    const int64_t total = (int64_t)B * C * HW;
    k_add_sample_bias<<<grid_stride_blocks(total), dim3(256), 0, cf_s(stream)>>>(h, bias, HW, total, relu);
    CF_LAUNCH_CHECK();
    return 0;
}

int cf_gmm_ctx_logprob(const float* x, const float* mG, const float* sG, const float* logw, const float* c, float* out,
                       float* lp_out, int B, int M, int K, int D, int HW, int64_t x_bstride, int accumulate,
                       cf_stream_t stream) {
    if (B == 0) return 0;
    CF_REQUIRE(x && mG && sG && logw && c && out && B >= 0 && M > 0 && K > 0 && D > 0 && HW > 0);
    int rc = gmm_ctx_fwd_launch<false>("cf_gmm_ctx_logprob", x, mG, sG, logw, c, out, lp_out, B, M, K, D, HW, x_bstride, accumulate,
                                       GmmTab{nullptr, nullptr, nullptr, nullptr, nullptr}, cf_s(stream));
    if (rc) return rc;
    CF_LAUNCH_CHECK();
    return 0;
}

int cf_gmm_ctx_tables(const float* sG, const float* cs_tab, float* inv_sig, float* dsig, float* lsum, int U, int MK, int D,
                      int HW, cf_stream_t stream) {
    if (U == 0) return 0;
    CF_REQUIRE(sG && cs_tab && inv_sig && lsum && U > 0 && MK > 0 && D > 0 && HW > 0);
    k_gmm_ctx_tables<<<dim3(U * MK), dim3(256), 0, cf_s(stream)>>>(sG, cs_tab, inv_sig, dsig, lsum, MK, D, HW);
    CF_LAUNCH_CHECK();
    return 0;
}

int cf_gmm_ctx_logprob_tab(const float* x, const float* mG, const float* inv_sig, const float* lsum, const float* logw,
                           const float* c, const int* ckey, const int* key, float* out, float* lp_out, int B, int M, int K,
                           int D, int HW, int64_t x_bstride, int accumulate, cf_stream_t stream) {
    if (B == 0) return 0;
    CF_REQUIRE(x && mG && inv_sig && lsum && logw && c && key && out && B >= 0 && M > 0 && K > 0 && D > 0 && HW > 0);
    int rc = gmm_ctx_fwd_launch<true>("cf_gmm_ctx_logprob_tab", x, mG, nullptr, logw, c, out, lp_out, B, M, K, D, HW, x_bstride,
                                      accumulate, GmmTab{inv_sig, nullptr, lsum, key, ckey}, cf_s(stream));
    if (rc) return rc;
    CF_LAUNCH_CHECK();
    return 0;
}

int cf_cond_gauss_sample(const float* c, const float* eps, float* x, float* logp, int B, int D, cf_stream_t stream) {
    if (B == 0) return 0;
    CF_REQUIRE(c && eps && x && logp && B >= 0 && D > 0);
    k_cond_gauss_sample<<<dim3(B), dim3(64), 0, cf_s(stream)>>>(c, eps, x, logp, D);
    CF_LAUNCH_CHECK();
    return 0;
}

int cf_sigmoid_ldj(const float* x, float* y, float* ldj, int B, int D, cf_stream_t stream) {
    if (B == 0) return 0;
    CF_REQUIRE(x && y && ldj && B >= 0 && D > 0);
    k_sigmoid_ldj<<<dim3(B), dim3(64), 0, cf_s(stream)>>>(x, y, ldj, D);
    CF_LAUNCH_CHECK();
    return 0;
}

int cf_conv1x1_ctx_bwd(const float* x, const float* m, const float* Wm, const float* gz, const float* gld, float* gx,
                       float* gm, int B, int C, int HW, int64_t x_bstride, int64_t gz_bstride, cf_stream_t stream) {
    if (B == 0) return 0;
    CF_REQUIRE(x && m && gz && gld && gx && gm && B >= 0 && C > 0 && HW > 0);
    if (int rc = launch_per_sample<k_conv1x1_ctx_bwd>(__func__, B, C, HW, CtxBwdLds(C, HW, 0, true).floats(), cf_s(stream), x, m, Wm, gz, gld,
                                                      gx, gm, C, HW, x_bstride, gz_bstride)) return rc;
    CF_LAUNCH_CHECK();
    return 0;
}

int cf_actnorm_ctx_bwd(const float* x, const float* m, const float* t, const float* logs, const float* gz, const float* gld,
                       float* gx, float* gm, int B, int C, int HW, int64_t x_bstride, int64_t gz_bstride, cf_stream_t stream) {
    if (B == 0) return 0;
    CF_REQUIRE(x && m && gz && gld && gx && gm && B >= 0 && C > 0 && HW > 0 && ((t == nullptr) == (logs == nullptr)));
    k_actnorm_ctx_bwd<<<dim3(B), dim3(256), 0, cf_s(stream)>>>(x, m, t, logs, gz, gld, gx, gm, C, HW, x_bstride, gz_bstride);
    CF_LAUNCH_CHECK();
    return 0;
}

// the input gradient through [Squeeze(2,2) ->] Conv1x1(c) -> ActNorm(c') in one launch; m1 / m2 NULL: a lone ActNorm / Conv1x1
int cf_affine_ctx_bwd_data(const float* gz, const float* m1, const float* Wm, const float* m2, const float* logs, float* gx,
                           int B, int C, int H, int W, int64_t gz_bstride, int out_unsqueeze, cf_stream_t stream) {
    if (B == 0) return 0;
    CF_REQUIRE(gz && gx && B >= 0 && C > 0 && C <= 256 && H > 0 && W > 0 && (m1 || !Wm) && (m2 || !logs) &&
               gz_bstride >= (int64_t)C * H * W && (!out_unsqueeze || C % 4 == 0));
    if (m1 && affine_wave_shape(C, H, W) && aligned16(gz, m1, Wm, m2, logs, gx) && gz_bstride % 4 == 0) {
        const dim3 grid((B + 3) / 4), blk(256);
#define CF_AFFB(CC, WW) do { if (out_unsqueeze) k_affine_ctx_bwd_wave<CC, WW, true><<<grid, blk, 0, cf_s(stream)>>>(gz, m1, Wm, m2, logs, gx, B, gz_bstride); \
                             else k_affine_ctx_bwd_wave<CC, WW, false><<<grid, blk, 0, cf_s(stream)>>>(gz, m1, Wm, m2, logs, gx, B, gz_bstride); } while (0)
        if (C == 16) CF_AFFB(16, 16); else if (C == 32) CF_AFFB(32, 8); else CF_AFFB(64, 4);
#undef CF_AFFB
        CF_LAUNCH_CHECK();
        return 0;
    }
    const int floats = CtxBwdLds(C, H * W, C, false, m1 != nullptr).floats();
    if (int rc = out_unsqueeze ? launch_per_sample<k_affine_ctx_bwd_data<true>>(__func__, B, C, H * W, floats, cf_s(stream), gz, m1, Wm, m2,
                                                                                logs, gx, C, H, W, gz_bstride)
                               : launch_per_sample<k_affine_ctx_bwd_data<false>>(__func__, B, C, H * W, floats, cf_s(stream), gz, m1, Wm, m2,
                                                                                 logs, gx, C, H, W, gz_bstride)) return rc;
    CF_LAUNCH_CHECK();
    return 0;
}

// [Squeeze(2,2) <-] Conv1x1(c) <- ActNorm(c') backwards in one launch; m1 / m2 NULL: a lone ActNorm / Conv1x1 inverse
int cf_affine_ctx_inv(const float* z, const float* m1, const float* Wm, const float* m2, const float* t, const float* logs,
                      float* x_out, int B, int C, int H, int W, int64_t z_bstride, int out_unsqueeze, cf_stream_t stream) {
    if (B == 0) return 0;
    CF_REQUIRE(z && x_out && (m1 || m2) && B >= 0 && C > 0 && C <= 256 && H > 0 && W > 0 && (m1 || !Wm) && (m2 || !logs) &&
               ((t == nullptr) == (logs == nullptr)) && z_bstride >= (int64_t)C * H * W && (!out_unsqueeze || C % 4 == 0));
    const int floats = CtxInvLds(C, H * W, m1 != nullptr).floats();
    if (int rc = out_unsqueeze ? launch_per_sample<k_affine_ctx_inv<true>>(__func__, B, C, H * W, floats, cf_s(stream), z, m1, Wm, m2, t, logs,
                                                                           x_out, C, H, W, z_bstride)
                               : launch_per_sample<k_affine_ctx_inv<false>>(__func__, B, C, H * W, floats, cf_s(stream), z, m1, Wm, m2, t, logs,
                                                                            x_out, C, H, W, z_bstride)) return rc;
    CF_LAUNCH_CHECK();
    return 0;
}

// the vector-Jacobian product of cf_affine_ctx_inv: gz = e^{l_b} (.) (W_b^-T gx); gx_unsqueezed: gx in the layout of the twin's
// out_unsqueeze output; m1 / m2 NULL as there
int cf_affine_ctx_inv_bwd_data(const float* gx, const float* m1, const float* Wm, const float* m2, const float* logs, float* gz,
                               int B, int C, int H, int W, int gx_unsqueezed, cf_stream_t stream) {
    if (B == 0) return 0;
    CF_REQUIRE(gx && gz && (m1 || m2) && B >= 0 && C > 0 && C <= 256 && H > 0 && W > 0 && (m1 || !Wm) && (m2 || !logs) &&
               (!gx_unsqueezed || C % 4 == 0));
    const int floats = CtxInvLds(C, H * W, m1 != nullptr).floats();
    const float* no_t = nullptr;
    const int64_t gbs = (int64_t)C * H * W;
    if (int rc = gx_unsqueezed ? launch_per_sample<k_affine_ctx_inv<true, true>>(__func__, B, C, H * W, floats, cf_s(stream), gx, m1, Wm, m2,
                                                                                 no_t, logs, gz, C, H, W, gbs)
                               : launch_per_sample<k_affine_ctx_inv<false, true>>(__func__, B, C, H * W, floats, cf_s(stream), gx, m1, Wm, m2,
                                                                                  no_t, logs, gz, C, H, W, gbs)) return rc;
    CF_LAUNCH_CHECK();
    return 0;
}

int cf_sample_channel_sums(const float* a, float* out, int B, int C, int HW, cf_stream_t stream) {
    if (B == 0) return 0;
    CF_REQUIRE(a && out && B >= 0 && C > 0 && HW > 0);
    const int64_t rows = (int64_t)B * C;
    k_sample_channel_sums<<<dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, cf_s(stream)>>>(a, out, HW, rows);
    CF_LAUNCH_CHECK();
    return 0;
}

int cf_relu_bwd(const float* x, const float* gy, float* out, int64_t n, cf_stream_t stream) {
    if (n == 0) return 0;
    CF_REQUIRE(x && gy && out && n >= 0);
    k_relu_bwd<<<grid_stride_blocks(n), dim3(256), 0, cf_s(stream)>>>(x, gy, out, n);
    CF_LAUNCH_CHECK();
    return 0;
}

int cf_gmm_ctx_bwd(const float* x, const float* mG, const float* sG, const float* logw, const float* c, const float* g,
                   const float* lp, float* gx, float* gc, int B, int M, int K, int D, int HW, int64_t x_bstride,
                   cf_stream_t stream) {
    if (B == 0) return 0;
    CF_REQUIRE(x && mG && sG && logw && c && g && gx && gc && B >= 0 && M > 0 && K > 0 && D > 0 && HW > 0);
    int rc = gmm_ctx_bwd_launch<false>("cf_gmm_ctx_bwd", x, mG, sG, logw, c, g, lp, gx, gc, B, M, K, D, HW, x_bstride,
                                       GmmTab{nullptr, nullptr, nullptr, nullptr, nullptr}, cf_s(stream));
    if (rc) return rc;
    CF_LAUNCH_CHECK();
    return 0;
}

int cf_gmm_ctx_bwd_tab(const float* x, const float* mG, const float* inv_sig, const float* dsig, const float* lsum,
                       const float* logw, const float* c, const int* key, const float* g, const float* lp, float* gx,
                       float* gc, int B, int M, int K, int D, int HW, int64_t x_bstride, cf_stream_t stream) {
    if (B == 0) return 0;
    CF_REQUIRE(x && mG && inv_sig && dsig && lsum && logw && c && key && g && gx && gc && B >= 0 && M > 0 && K > 0 && D > 0 && HW > 0);
    int rc = gmm_ctx_bwd_launch<true>("cf_gmm_ctx_bwd_tab", x, mG, nullptr, logw, c, g, lp, gx, gc, B, M, K, D, HW, x_bstride,
                                      GmmTab{inv_sig, dsig, lsum, key, nullptr}, cf_s(stream));
    if (rc) return rc;
    CF_LAUNCH_CHECK();
    return 0;
}

// d/dx alone of either form (FlowSequential.score with a context): inv_sig / lsum / key select the table form, sG the direct
// one; the kernels of cf_gmm_ctx_bwd / cf_gmm_ctx_bwd_tab with everything that leads to gc compiled out - gx is bitwise equal.
int cf_gmm_ctx_bwd_data(const float* x, const float* mG, const float* sG, const float* inv_sig, const float* lsum,
                        const float* logw, const float* c, const int* key, const float* g, const float* lp, float* gx, int B,
                        int M, int K, int D, int HW, int64_t x_bstride, cf_stream_t stream) {
    if (B == 0) return 0;
    const bool tab = inv_sig != nullptr || lsum != nullptr || key != nullptr;
    CF_REQUIRE(x && mG && logw && c && g && gx && B >= 0 && M > 0 && K > 0 && D > 0 && HW > 0 &&
               (tab ? (inv_sig && lsum && key) : sG != nullptr));
    int rc = tab ? gmm_ctx_bwd_launch<true, true>("cf_gmm_ctx_bwd_data", x, mG, nullptr, logw, c, g, lp, gx, nullptr, B, M, K, D, HW,
                                                  x_bstride, GmmTab{inv_sig, nullptr, lsum, key, nullptr}, cf_s(stream))
                 : gmm_ctx_bwd_launch<false, true>("cf_gmm_ctx_bwd_data", x, mG, sG, logw, c, g, lp, gx, nullptr, B, M, K, D, HW,
                                                   x_bstride, GmmTab{nullptr, nullptr, nullptr, nullptr, nullptr}, cf_s(stream));
    if (rc) return rc;
    CF_LAUNCH_CHECK();
    return 0;
}

int cf_gmm_ctx_pgrad_tab(const float* x, const float* mG, const float* inv_sig, const float* dsig, const float* c,
                          const int* key, const float* r, float* pgm, float* pgs, int B, int M, int K, int D, int HW,
                          int64_t x_bstride, int slab, cf_stream_t stream) {
    if (B == 0) return 0;
    CF_REQUIRE(x && mG && inv_sig && dsig && c && key && r && pgm && pgs && B >= 0 && M > 0 && K > 0 && D > 0 && HW > 0 && slab > 0);
    const int N = D * HW, nb = (B + slab - 1) / slab;
    CF_REQUIRE(M * K <= 65535 && nb <= 65535);
    k_gmm_ctx_pgrad<<<dim3((N + 255) / 256, M * K, nb), dim3(256), 0, cf_s(stream)>>>(
        x, mG, c, r, pgm, pgs, B, M * K, D, HW, x_bstride, slab, GmmTab{inv_sig, dsig, nullptr, key, nullptr});
    CF_LAUNCH_CHECK();
    return 0;
}

int cf_add_repeat(float* h, const float* x, int B, int C2, int C, int HW, cf_stream_t stream) {
    if (B == 0) return 0;
    CF_REQUIRE(h && x && B >= 0 && C2 > 0 && C > 0 && HW > 0);
    const int64_t total = (int64_t)B * C2 * HW;
    k_add_repeat<<<grid_stride_blocks(total), dim3(256), 0, cf_s(stream)>>>(h, x, C2, C, HW, total);
    CF_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
