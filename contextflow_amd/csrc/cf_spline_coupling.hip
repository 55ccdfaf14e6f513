// SplineCoupling: z = [x0 | RQS(x1; h)] with the knots of every element taken from the conditioner output h = NN(x0)
// (monotone rational-quadratic spline with linear tails: layers/splines/rational_quadratic.py:21-176, the per-element
// arithmetic k_spline_tables / k_spline of cf_spline.hip state; conditioner layout: layers/activations.py:140).
//
// h (B, D (3K-1), HW): channel c (3K-1) + j belongs to data channel c - j < K unnormalised widths, K <= j < 2K heights,
// 2K <= j < 3K-1 interior derivatives.  Consecutive lanes walk pixels, so each of the 3K-1 parameter reads of an element is
// a row of h.  A lane owns four consecutive elements of its sample: their raw parameters are read into registers (one
// dwordx4 per parameter row where the pixel count, the strides and the pointers allow it, four dwords otherwise - the same
// elements, the same arithmetic and the same order of the log-det sum in both forms), and the knot tables - softmax,
// cumulative sums, softplus - are formed there and never stored.  One workgroup per sample; the log-det is reduced with
// wave shuffles and one LDS hop, written by one thread: no atomics, two launches give the same bits.
//
// Backward: the tables and the bin are recomputed from h and x1; the gradient goes through the RQ map, its log-derivative,
// the floor + softmax + cumulative sum of widths and heights and the softplus of the derivatives, and every raw parameter
// of an element is written once (zeros outside the tails): no atomics either.
#include "cf_common.h"
#include <math.h>

#pragma clang fp contract(off)      // one rounding per operation in every form of the kernels: the vector and the scalar form agree bitwise

namespace {

// the per-element arithmetic also compiles for the host (a stand-alone program can check it against a reference)
#define CF_HD __host__ __device__ __forceinline__

// (doubles: the forward and the inverse work in fp32, the backward forms its knots and the map's derivatives in fp64 - see
// spline_elem_bwd - and each takes the constants rounded to its own type)
constexpr double kMinW = 1e-3, kMinH = 1e-3, kMinD = 1e-3;
constexpr double kDerivCst = 0.5397424172369522;      // log(exp(1 - kMinD) - 1): an unnormalised derivative of 0 gives a derivative of 1
constexpr int kMaxBins = 16;
constexpr int kPer = 4;                               // elements per lane and pass

CF_HD float exp_t(float v) { return expf(v); }
CF_HD double exp_t(double v) { return exp(v); }
CF_HD float softplus1(float v) { return v > 20.f ? v : log1pf(expf(v)); }
CF_HD double softplus1(double v) { return v > 20.0 ? v : log1p(exp(v)); }
CF_HD float sigmoid1(float v) { return v > 20.f ? 1.f : 1.f / (1.f + expf(-v)); }

// One parameter row of one element: u (raw, K of KMAX entries used) becomes the softmax p in place, and the knots
// c_0 = -bound, c_k = 2 bound sum_{j<k} (mn + (1 - mn K) p_j) - bound, c_K = bound are walked once, in the type T.
// SEARCH: idx = the last k < K with v >= c_k (searchsorted: the 1e-6 on the last knot keeps v = bound in bin K-1); otherwise
// idx is given.  lo, hi = c_idx, c_idx+1;  slo, shi = sum_{j<idx} p_j, sum_{j<=idx} p_j (the backward's softmax dot).
template <int KMAX, bool SEARCH, typename T>
CF_HD void knot_walk(float (&u)[KMAX], int K, T bound, T mn, T v, int& idx, T& lo, T& hi, T& slo, T& shi) {
    float mx = u[0];
#pragma unroll
    for (int k = 1; k < KMAX; ++k)
        if (k < K) mx = fmaxf(mx, u[k]);
    T e[KMAX];
    T sum = 0;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
        if (k < K) { e[k] = exp_t((T)u[k] - (T)mx); sum += e[k]; }
    const T scale = (T)1 - mn * (T)K;
    T cum = 0, cp = 0, prev = -bound;
    if (SEARCH) idx = 0;
    lo = -bound; hi = bound; slo = 0; shi = 1;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
        if (k < K) {
            const T p = e[k] / sum;
            u[k] = (float)p;
            cum += mn + scale * p;
            const T nxt = (k == K - 1) ? bound : (T)2 * bound * cum - bound;
            const T cpn = cp + p;
            const bool take = SEARCH ? (v >= prev) : (k == idx);
            if (take) { if (SEARCH) idx = k; lo = prev; hi = nxt; slo = cp; shi = cpn; }
            prev = nxt; cp = cpn;
        }
}

// raw[idx - 1] and raw[idx] of the interior derivatives (K - 1 entries), 0 at the boundary knots: with kDerivCst the boundary
// derivatives come out of the same expression as 1
template <int KMAX, typename T>
CF_HD void deriv_pick(const float (&ud)[KMAX], int K, int idx, T& d0, T& d1) {
    float r0 = 0.f, r1 = 0.f;
#pragma unroll
    for (int m = 0; m < KMAX - 1; ++m)
        if (m < K - 1) { if (m == idx - 1) r0 = ud[m]; if (m == idx) r1 = ud[m]; }
    d0 = idx == 0 ? (T)1 : (T)kMinD + softplus1((T)r0 + (T)kDerivCst);
    d1 = idx == K - 1 ? (T)1 : (T)kMinD + softplus1((T)r1 + (T)kDerivCst);
}

// the raw parameters of kPer consecutive elements e0 .. e0+3 of sample b (element e = c HW + p)
template <int KMAX>
struct Raw {
    float w[kPer][KMAX], h[kPer][KMAX], d[kPer][KMAX];      // d: K - 1 entries used
};

template <int KMAX, bool VEC>
__device__ __forceinline__ void load_raw(Raw<KMAX>& r, const float* __restrict__ hb, int e0, int per, int HW, int K) {
    const int nj = 3 * K - 1;
    if (VEC) {                                              // HW % 4 == 0: the four elements share their channel
        const float* base = hb + (int64_t)(e0 / HW) * nj * HW + (e0 % HW);
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {                   // the register of an entry is fixed at compile time, its row is not
            float4 qw = make_float4(0.f, 0.f, 0.f, 0.f), qh = qw, qd = qw;
            if (k < K) {
                qw = *reinterpret_cast<const float4*>(base + (int64_t)k * HW);
                qh = *reinterpret_cast<const float4*>(base + (int64_t)(K + k) * HW);
            }
            if (k < K - 1) qd = *reinterpret_cast<const float4*>(base + (int64_t)(2 * K + k) * HW);
            r.w[0][k] = qw.x; r.w[1][k] = qw.y; r.w[2][k] = qw.z; r.w[3][k] = qw.w;
            r.h[0][k] = qh.x; r.h[1][k] = qh.y; r.h[2][k] = qh.z; r.h[3][k] = qh.w;
            r.d[0][k] = qd.x; r.d[1][k] = qd.y; r.d[2][k] = qd.z; r.d[3][k] = qd.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < kPer; ++i) {
            const int e = e0 + i;
            const bool ok = e < per;
            const float* base = hb + (ok ? (int64_t)(e / HW) * nj * HW + (e % HW) : 0);
#pragma unroll
            for (int k = 0; k < KMAX; ++k) {
                r.w[i][k] = (ok && k < K) ? base[(int64_t)k * HW] : 0.f;
                r.h[i][k] = (ok && k < K) ? base[(int64_t)(K + k) * HW] : 0.f;
                r.d[i][k] = (ok && k < K - 1) ? base[(int64_t)(2 * K + k) * HW] : 0.f;
            }
        }
    }
}

template <bool VEC>
__device__ __forceinline__ void load4(float (&v)[kPer], const float* __restrict__ p, int e0, int per) {
    if (VEC) {
        const float4 q = *reinterpret_cast<const float4*>(p + e0);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int i = 0; i < kPer; ++i) v[i] = e0 + i < per ? p[e0 + i] : 0.f;
    }
}

template <bool VEC>
__device__ __forceinline__ void store4(const float (&v)[kPer], float* __restrict__ p, int e0, int per) {
    if (VEC) {
        *reinterpret_cast<float4*>(p + e0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int i = 0; i < kPer; ++i)
            if (e0 + i < per) p[e0 + i] = v[i];
    }
}

// the RQ map of one element inside the tails: v -> out (forward: v = x1, inverse: v = z1) and the forward log-derivative at
// the x1 of the pair
template <int KMAX, bool INV>
CF_HD void spline_elem(float (&uw)[KMAX], float (&uh)[KMAX], const float (&ud)[KMAX], int K, float bound, float v, float& out,
                       float& lad) {
    int idx;
    float w0, w1, h0, h1, s0, s1, d0, d1;
    if (INV) {
        knot_walk<KMAX, true, float>(uh, K, bound, (float)kMinH, v, idx, h0, h1, s0, s1);
        knot_walk<KMAX, false, float>(uw, K, bound, (float)kMinW, v, idx, w0, w1, s0, s1);
    } else {
        knot_walk<KMAX, true, float>(uw, K, bound, (float)kMinW, v, idx, w0, w1, s0, s1);
        knot_walk<KMAX, false, float>(uh, K, bound, (float)kMinH, v, idx, h0, h1, s0, s1);
    }
    deriv_pick<KMAX, float>(ud, K, idx, d0, d1);
    const float w = w1 - w0, h = h1 - h0;
    const float delta = h / w;
    const float s2 = d0 + d1 - 2.f * delta;
    float th;
    if (INV) {
        const float u = v - h0;
        const float a = u * s2 + h * (delta - d0);
        const float bq = h * d0 - u * s2;
        const float c = -delta * u;
        th = (2.f * c) / (-bq - sqrtf(fmaxf(bq * bq - 4.f * a * c, 0.f)));
        out = th * w + w0;
    } else {
        th = (v - w0) / w;
        out = h0 + h * (delta * th * th + d0 * th * (1.f - th)) / (delta + s2 * th * (1.f - th));
    }
    const float om = 1.f - th;
    const float den = delta + s2 * th * om;
    lad = logf(delta * delta * (d1 * th * th + 2.f * delta * th * om + d0 * om * om)) - 2.f * logf(den);
}

template <bool INV, int KMAX, bool VEC, int NT>
__global__ __launch_bounds__(NT) void k_spline_coupling(const float* __restrict__ x, const float* __restrict__ h,
                                                        float* __restrict__ z, float* __restrict__ ldj, int per, int HW, int K,
                                                        float bound, int64_t xbs) {
    __shared__ float red[NT / 64];
    const int b = blockIdx.x;
    const float* xb = x + (int64_t)b * xbs;
    const float* hb = h + (int64_t)b * per * (3 * K - 1);
    float* zb = z + (int64_t)b * 2 * per;
    float acc = 0.f;
    for (int e0 = threadIdx.x * kPer; e0 < per; e0 += NT * kPer) {
        float v[kPer], o[kPer];
        load4<VEC>(v, xb, e0, per);
        store4<VEC>(v, zb, e0, per);                          // z0 = x0
        load4<VEC>(v, xb + per, e0, per);
        Raw<KMAX> r;
        load_raw<KMAX, VEC>(r, hb, e0, per, HW, K);
#pragma unroll
        for (int i = 0; i < kPer; ++i) {
            float out, lad;
            spline_elem<KMAX, INV>(r.w[i], r.h[i], r.d[i], K, bound, v[i], out, lad);
            const bool inside = v[i] >= -bound && v[i] <= bound;            // the tails are the identity with log-derivative 0
            o[i] = inside ? out : v[i];
            if (VEC || e0 + i < per) acc += inside ? lad : 0.f;
        }
        store4<VEC>(o, zb + per, e0, per);
    }
    if (!INV || ldj != nullptr) {        // (inverse: the forward log-det at the recovered input, when asked for)
        acc = cf_block_sum<NT / 64>(acc, red);
        if (threadIdx.x == 0) ldj[b] = acc;
    }
}

// gradient of one parameter row's softmax entries, in place: u holds p (knot_walk); a0 / a1 = the gradients w.r.t. the knots
// c_idx / c_idx+1 times 2 bound (1 - mn K), 0 where that knot is a boundary.  d c_k / d p_j = [j < k], so
// g_j = p_j ([j < idx] a0 + [j <= idx] a1 - dot) with dot = a0 sum_{j<idx} p_j + a1 sum_{j<=idx} p_j.
template <int KMAX>
CF_HD void softmax_grad(float (&u)[KMAX], int K, int idx, float a0, float a1, float dot, bool inside) {
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
        if (k < K) {
            const float up = (k < idx ? a0 : 0.f) + (k <= idx ? a1 : 0.f);
            u[k] = inside ? u[k] * (up - dot) : 0.f;
        }
}

// backward of one element: uw, uh, ud (raw) become the gradient w.r.t. themselves, in place; returns the gradient w.r.t. x1.
// gz1 = d/d z1, gl = d/d (the sample's log-det).  Outside the tails: gz1 and zeros.
// The knots, the position theta = (x1 - w0) / W in the bin and the reverse sweep through the map are formed in fp64: a bin may
// be as narrow as 2e-3 bound, a knot carries the rounding of a cumulative sum over all bins in front of it, and the gradients
// grow like 1 / W - in fp32 the largest entries of gx and gh are the least accurate ones (1e-4 .. 1e-3 of the largest entry,
// where the chain through the softmax, in fp32 from the rounded p, adds 1e-7).  Costs 2 K fp64 exponentials per element.
template <int KMAX>
CF_HD float spline_elem_bwd(float (&uw)[KMAX], float (&uh)[KMAX], float (&ud)[KMAX], int K, float bound_f, float vf, float gz1,
                            float gl_f) {
    typedef double T;
    const T bound = bound_f, v = vf, a = gz1, gl = gl_f;
    int idx;
    T w0, w1, h0, h1, sw0, sw1, sh0, sh1, d0, d1;
    knot_walk<KMAX, true, T>(uw, K, bound, (T)kMinW, v, idx, w0, w1, sw0, sw1);
    knot_walk<KMAX, false, T>(uh, K, bound, (T)kMinH, v, idx, h0, h1, sh0, sh1);
    deriv_pick<KMAX, T>(ud, K, idx, d0, d1);
    const bool inside = vf >= -bound_f && vf <= bound_f;
    // forward values
    const T Wd = w1 - w0, Hd = h1 - h0, delta = Hd / Wd;
    const T th = (v - w0) / Wd, om = 1 - th, t = th * om;
    const T s2 = d0 + d1 - 2 * delta;
    const T A = delta * th * th + d0 * t;
    const T num = Hd * A, den = delta + s2 * t;
    const T P = d1 * th * th + 2 * delta * t + d0 * om * om;
    // reverse sweep of  G = gz1 z1 + gl lad,  z1 = h0 + num / den,  lad = 2 log delta + log P - 2 log den
    const T g_num = a / den;
    const T g_den = -(a * num / den + 2 * gl) / den;
    const T g_P = gl / P;
    const T g_A = g_num * Hd;
    const T g_s2 = g_den * t;
    const T g_delta = 2 * gl / delta + g_A * th * th + g_den + g_P * 2 * t - 2 * g_s2;
    const T g_t = g_A * d0 + g_den * s2 + g_P * 2 * delta;
    const T g_om = g_P * 2 * d0 * om + g_t * th;
    const T g_th = g_A * 2 * delta * th + g_P * 2 * d1 * th + g_t * om - g_om;
    const T g_d0 = g_A * t + g_P * om * om + g_s2;
    const T g_d1 = g_P * th * th + g_s2;
    const T g_H = g_num * A + g_delta / Wd;
    const T g_W = -(g_delta * delta + g_th * th) / Wd;
    const T g_x = g_th / Wd;
    const T g_w0 = -g_x - g_W, g_w1 = g_W;
    const T g_h0 = a - g_H, g_h1 = g_H;
    const bool first = idx == 0, last = idx == K - 1;
    const T cw = 2 * bound * (1 - (T)kMinW * K), ch = 2 * bound * (1 - (T)kMinH * K);
    const T aw0 = first ? 0 : cw * g_w0, aw1 = last ? 0 : cw * g_w1, ah0 = first ? 0 : ch * g_h0, ah1 = last ? 0 : ch * g_h1;
    // dot products of the softmax rule in fp64 (they cancel against a0, a1), the K products per row in fp32
    softmax_grad<KMAX>(uw, K, idx, (float)aw0, (float)aw1, (float)(aw0 * sw0 + aw1 * sw1), inside);
    softmax_grad<KMAX>(uh, K, idx, (float)ah0, (float)ah1, (float)(ah0 * sh0 + ah1 * sh1), inside);
#pragma unroll
    for (int m = 0; m < KMAX - 1; ++m)
        if (m < K - 1) {
            const float up = m == idx - 1 ? (float)g_d0 : (m == idx ? (float)g_d1 : 0.f);
            ud[m] = (inside && (m == idx - 1 || m == idx)) ? up * sigmoid1(ud[m] + (float)kDerivCst) : 0.f;
        }
    return inside ? (float)g_x : gz1;
}

template <int KMAX, bool VEC, int NT>
__global__ __launch_bounds__(NT) void k_spline_coupling_bwd(const float* __restrict__ x, const float* __restrict__ h,
                                                            const float* __restrict__ gz, const float* __restrict__ gld,
                                                            float* __restrict__ gx, float* __restrict__ gh, int per, int HW, int K,
                                                            float bound, int64_t xbs, int64_t gzbs) {
    const int b = blockIdx.x;
    const int nj = 3 * K - 1;
    const float* xb = x + (int64_t)b * xbs;
    const float* gzb = gz + (int64_t)b * gzbs;
    const float* hb = h + (int64_t)b * per * nj;
    float* gxb = gx + (int64_t)b * 2 * per;
    float* ghb = gh + (int64_t)b * per * nj;
    const float gl = gld[b];
    for (int e0 = threadIdx.x * kPer; e0 < per; e0 += NT * kPer) {
        float v[kPer], g[kPer], o[kPer];
        load4<VEC>(g, gzb, e0, per);
        store4<VEC>(g, gxb, e0, per);                         // gx0 = gz0 (the conditioner's part is the caller's)
        load4<VEC>(v, xb + per, e0, per);
        load4<VEC>(g, gzb + per, e0, per);
        Raw<KMAX> r;
        load_raw<KMAX, VEC>(r, hb, e0, per, HW, K);
#pragma unroll
        for (int i = 0; i < kPer; ++i) o[i] = spline_elem_bwd<KMAX>(r.w[i], r.h[i], r.d[i], K, bound, v[i], g[i], gl);
        store4<VEC>(o, gxb + per, e0, per);
        // r now holds the gradient of every raw parameter of the four elements: written row by row, as they were read
        if (VEC) {
            float* base = ghb + (int64_t)(e0 / HW) * nj * HW + (e0 % HW);
#pragma unroll
            for (int k = 0; k < KMAX; ++k) {
                if (k < K) {
                    *reinterpret_cast<float4*>(base + (int64_t)k * HW) = make_float4(r.w[0][k], r.w[1][k], r.w[2][k], r.w[3][k]);
                    *reinterpret_cast<float4*>(base + (int64_t)(K + k) * HW) = make_float4(r.h[0][k], r.h[1][k], r.h[2][k], r.h[3][k]);
                }
                if (k < K - 1)
                    *reinterpret_cast<float4*>(base + (int64_t)(2 * K + k) * HW) = make_float4(r.d[0][k], r.d[1][k], r.d[2][k], r.d[3][k]);
            }
        } else {
#pragma unroll
            for (int i = 0; i < kPer; ++i) {
                const int e = e0 + i;
                if (e < per) {
                    float* base = ghb + (int64_t)(e / HW) * nj * HW + (e % HW);
#pragma unroll
                    for (int k = 0; k < KMAX; ++k) {
                        if (k < K) { base[(int64_t)k * HW] = r.w[i][k]; base[(int64_t)(K + k) * HW] = r.h[i][k]; }
                        if (k < K - 1) base[(int64_t)(2 * K + k) * HW] = r.d[i][k];
                    }
                }
            }
        }
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <bool INV, int KMAX, bool VEC>
void launch_fwd(const float* x, const float* h, float* z, float* ldj, int B, int per, int HW, int K, float bound, int64_t xbs,
                hipStream_t st) {
    if (per > 256 * kPer) k_spline_coupling<INV, KMAX, VEC, 256><<<dim3(B), dim3(256), 0, st>>>(x, h, z, ldj, per, HW, K, bound, xbs);
    else k_spline_coupling<INV, KMAX, VEC, 64><<<dim3(B), dim3(64), 0, st>>>(x, h, z, ldj, per, HW, K, bound, xbs);
}

template <int KMAX, bool VEC>
void launch_bwd(const float* x, const float* h, const float* gz, const float* gld, float* gx, float* gh, int B, int per, int HW,
                int K, float bound, int64_t xbs, int64_t gzbs, hipStream_t st) {
    if (per > 256 * kPer)
        k_spline_coupling_bwd<KMAX, VEC, 256><<<dim3(B), dim3(256), 0, st>>>(x, h, gz, gld, gx, gh, per, HW, K, bound, xbs, gzbs);
    else
        k_spline_coupling_bwd<KMAX, VEC, 64><<<dim3(B), dim3(64), 0, st>>>(x, h, gz, gld, gx, gh, per, HW, K, bound, xbs, gzbs);
}

}  // namespace

extern "C" {

int cf_spline_coupling(const float* x, const float* h, float* z, float* ldj, int B, int C, int HW, int K, float tail_bound,
                       int64_t x_bstride, int inverse, cf_stream_t stream) {
    if (B == 0) return 0;                       // empty batch: nothing to do (pointers may be null)
    if (K < 2 || K > kMaxBins) { cf_set_error("cf_spline_coupling: K=%d unsupported (2..%d)", K, kMaxBins); return CF_ERR_UNSUPPORTED; }
    CF_REQUIRE(x && h && z && (inverse || ldj) && B > 0 && C >= 2 && C % 2 == 0 && HW > 0 && tail_bound > 0.f);
    CF_REQUIRE(x_bstride >= (int64_t)C * HW && (int64_t)(C / 2) * HW * (3 * K - 1) < (1ll << 31));
    const int per = (C / 2) * HW;
    const bool vec = HW % 4 == 0 && x_bstride % 4 == 0 && aligned16(x) && aligned16(h) && aligned16(z);
    hipStream_t st = cf_s(stream);
#define CF_SC_FWD(INV, KMAX)                                                                                           \
    do {                                                                                                               \
        if (vec) launch_fwd<INV, KMAX, true>(x, h, z, ldj, B, per, HW, K, tail_bound, x_bstride, st);                  \
        else launch_fwd<INV, KMAX, false>(x, h, z, ldj, B, per, HW, K, tail_bound, x_bstride, st);                     \
    } while (0)
    if (inverse) { if (K <= 8) CF_SC_FWD(true, 8); else CF_SC_FWD(true, 16); }
    else { if (K <= 8) CF_SC_FWD(false, 8); else CF_SC_FWD(false, 16); }
#undef CF_SC_FWD
    CF_LAUNCH_CHECK();
    return 0;
}

int cf_spline_coupling_bwd(const float* x, const float* h, const float* gz, const float* gld, float* gx, float* gh, int B, int C,
                           int HW, int K, float tail_bound, int64_t x_bstride, int64_t gz_bstride, cf_stream_t stream) {
    if (B == 0) return 0;
    if (K < 2 || K > kMaxBins) { cf_set_error("cf_spline_coupling_bwd: K=%d unsupported (2..%d)", K, kMaxBins); return CF_ERR_UNSUPPORTED; }
    CF_REQUIRE(x && h && gz && gld && gx && gh && B > 0 && C >= 2 && C % 2 == 0 && HW > 0 && tail_bound > 0.f);
    CF_REQUIRE(x_bstride >= (int64_t)C * HW && gz_bstride >= (int64_t)C * HW && (int64_t)(C / 2) * HW * (3 * K - 1) < (1ll << 31));
    const int per = (C / 2) * HW;
    const bool vec = HW % 4 == 0 && x_bstride % 4 == 0 && gz_bstride % 4 == 0 && aligned16(x) && aligned16(h) && aligned16(gz) &&
                     aligned16(gx) && aligned16(gh);
    hipStream_t st = cf_s(stream);
    if (K <= 8) {
        if (vec) launch_bwd<8, true>(x, h, gz, gld, gx, gh, B, per, HW, K, tail_bound, x_bstride, gz_bstride, st);
        else launch_bwd<8, false>(x, h, gz, gld, gx, gh, B, per, HW, K, tail_bound, x_bstride, gz_bstride, st);
    } else {
        if (vec) launch_bwd<16, true>(x, h, gz, gld, gx, gh, B, per, HW, K, tail_bound, x_bstride, gz_bstride, st);
        else launch_bwd<16, false>(x, h, gz, gld, gx, gh, B, per, HW, K, tail_bound, x_bstride, gz_bstride, st);
    }
    CF_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
