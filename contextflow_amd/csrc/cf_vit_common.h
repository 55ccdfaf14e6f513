// Shared by the sources of the transformer coupling (cf_vit_fused.hip) and of the one-kernel transformer flow steps
// (cf_vit_step.hip: the cf_vit_step_* entry points and the wave form, cf_vit_rs.hip: the row-split form, cf_vit_rs_bwd.h: the
// backward): the flat parameter layout, the limits and sizes every form agrees on, the device helpers they have in common, the
// fused attention matrices, and the per-form host functions behind the entry points.
#pragma once
#include "cf_common.h"

// ---- the row-split form, as the entry points of cf_vit_step.hip call it (defined in cf_vit_rs.hip; arguments arrive validated;
// not part of the library's exports)
#define CF_VIT_LOCAL __attribute__((visibility("hidden")))
CF_VIT_LOCAL int64_t vit_rs_ws_floats(int depth);
CF_VIT_LOCAL int vit_rs_prepare_batch(int n, const float* const* Wm, const float* const* t, const float* const* logs,
                                      const float* const* flat, const float* pos, void* const* ws, float* const* winv, void* const* wsb,
                                      int depth, cf_stream_t stream);
CF_VIT_LOCAL int vit_rs_fwd(const float* x, float* z, float* ldj_acc, const float* ws, float* h_out, float* xtape, int B, int depth,
                            int64_t xbs, cf_stream_t stream);
CF_VIT_LOCAL int vit_rs_fwd_chain(const float* x, float* z, float* ldj_acc, const void* const* ws, int n, int B, int depth, int64_t xbs,
                                  cf_stream_t stream);

namespace {

constexpr int kVitMaxDepth = 6;          // the backward kernel parks the residual stream of <= 6 layer boundaries in LDS (RSB::LDS_FLOATS)
constexpr int kVitChain = 8;             // consecutive steps of one k_vit_step_rs_chain launch
constexpr int kVitPrepBatch = 16;        // flow steps per launch of the batched pack kernels

// geometry of the one-kernel steps: SMAP - C = 26 channels on 8 x 1 windows, patch (2, 1), dim = 2C, one head of 64
inline bool vit_step_geometry_ok(int C, int H, int W, int p1, int p2, int dim, int dim_head, int heads) {
    return C == 26 && H == 8 && W == 1 && p1 == 2 && p2 == 1 && dim == 2 * C && dim_head == 64 && heads == 1;
}
// token columns of the residual-stream tape ([depth + 1][2C][T]): 4 per sample, the batch rounded up to the wave form's 32 samples
__host__ __device__ constexpr int64_t vit_tape_tokens(int B) { return 4ll * ((B + 31) / 32 * 32); }

// Flat parameter vector of a SimpleViT conditioner (TransCoupling._flat_params_build writes it, every pack kernel reads it), as
// offsets in floats:
//   ln0.w(pd) ln0.b(pd) We(dim x pd) be(dim) ln1.w(dim) ln1.b(dim)                                      front: to_patch_embedding
//   depth x [ ga ba (attention norm) | Wq Wk Wv (head x dim each) | Wo (dim x head) | gf bf (feed-forward norm) | W1 b1 W2 b2 ]
//   lnO.w lnO.b                                                                                           transformer.norm
// The per-layer members are relative to layer(l).
struct VitFlat {
    int pd, dim, head;
    __host__ __device__ constexpr VitFlat(int pd_, int dim_, int head_ = 64) : pd(pd_), dim(dim_), head(head_) {}
    __host__ __device__ constexpr int ln0_w() const { return 0; }
    __host__ __device__ constexpr int ln0_b() const { return pd; }
    __host__ __device__ constexpr int we() const { return 2 * pd; }
    __host__ __device__ constexpr int be() const { return we() + dim * pd; }
    __host__ __device__ constexpr int ln1_w() const { return be() + dim; }
    __host__ __device__ constexpr int ln1_b() const { return ln1_w() + dim; }
    __host__ __device__ constexpr int layer0() const { return ln1_b() + dim; }
    __host__ __device__ constexpr int ga() const { return 0; }
    __host__ __device__ constexpr int ba() const { return dim; }
    __host__ __device__ constexpr int wq() const { return 2 * dim; }                      // to_qkv (3 head x dim) starts here
    __host__ __device__ constexpr int wk() const { return wq() + head * dim; }
    __host__ __device__ constexpr int wv() const { return wk() + head * dim; }
    __host__ __device__ constexpr int wo() const { return wv() + head * dim; }
    __host__ __device__ constexpr int gf() const { return wo() + dim * head; }
    __host__ __device__ constexpr int bf() const { return gf() + dim; }
    __host__ __device__ constexpr int w1() const { return bf() + dim; }
    __host__ __device__ constexpr int b1() const { return w1() + dim * dim; }
    __host__ __device__ constexpr int w2() const { return b1() + dim; }
    __host__ __device__ constexpr int b2() const { return w2() + dim * dim; }
    __host__ __device__ constexpr int layer_stride() const { return b2() + dim; }
    __host__ __device__ constexpr int layer(int l) const { return layer0() + l * layer_stride(); }
    __host__ __device__ constexpr int lno_w(int depth) const { return layer(depth); }
    __host__ __device__ constexpr int lno_b(int depth) const { return lno_w(depth) + dim; }
    __host__ __device__ constexpr int total(int depth) const { return lno_b(depth) + dim; }
};

// ---- device helpers of the step kernels -------------------------------------------------------------------------------
typedef __amdgpu_buffer_rsrc_t rsrc_t;

__host__ __device__ constexpr int ngrp(int ks) { return (ks + 3) / 4; }          // groups of 4 k-steps: one 16-byte fragment per lane

__device__ __forceinline__ rsrc_t make_rsrc(const float* ws, int floats) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(ws), 0, floats * 4, 0x00020000);
}
__device__ __forceinline__ float4 frag(rsrc_t rs, int lane, int foff) {
#ifdef CF_ABL_VS_NOFRAG           // probe build of the wave form (tools/dev/make_abl.py)
    return make_float4(1e-3f * lane, 2e-3f, 3e-3f * foff, 1e-3f);
#endif
    typedef int i32x4_t __attribute__((ext_vector_type(4)));
    const i32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(rs, lane * 16, foff * 4, 0);
    return make_float4(__int_as_float(v.x), __int_as_float(v.y), __int_as_float(v.z), __int_as_float(v.w));
}
__device__ __forceinline__ float f4e(const float4& v, int e) { return e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w; }

template <int CTRL> __device__ __forceinline__ float quad(float v) {          // DPP quad permutation of the 4 tokens of a sample
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}
template <int M> __device__ __forceinline__ float tok_xor(float v) {
    if constexpr (M == 0) return v;
    else if constexpr (M == 1) return quad<0xB1>(v);      // [1,0,3,2]
    else if constexpr (M == 2) return quad<0x4E>(v);      // [2,3,0,1]
    else return quad<0x1B>(v);                            // [3,2,1,0]
}

// one thread of a forward pack kernel: ws[0] = ldj_const = H*W*log|det Wm| + sum_c logs   (conv1x1.py:53 + actnorm.py:58;
// ws[1] holds log|det Wm| from cf_slogdet_inverse)
template <class V> __device__ __forceinline__ void pack_ldj_const(float* __restrict__ ws, const float* __restrict__ logs) {
    float s = 0.f;
    for (int c = 0; c < V::C; ++c) s += logs[c];
    ws[0] = (float)V::HW * ws[1] + s;
}

// ---- fused attention matrices -----------------------------------------------------------------------------------------
// Formed ONCE per parameter version in fp64 and rounded to fp32 once.  A single head of HEAD = 64 on a DIM = 52-wide stream makes
// the score and the value / output maps factor through the stream (simple_vit.py:56-68): with u = g (.) n + b the attention
// pre-norm output,
//     q_i . k_j / 8  =  (M1 n_i + c1) . n_j  + terms without n_j (equal for the four keys of a query: they leave the softmax),
//         M1 = diag(g) Wk^T Wq diag(g) / 8,   c1 = diag(g) Wk^T Wq b / 8,
//     to_out(sum_j p_ij Wv u_j)  =  M2 (sum_j p_ij n_j) + c2,     M2 = Wout Wv diag(g),   c2 = Wout Wv b     (sum_j p_ij = 1).
// k_vit_fuse writes, per layer, [M1 (DIM x DIM, row-major) | c1 (DIM) | M2 (DIM x DIM) | c2 (DIM)] floats; the pack kernels
// of the two step kernels copy entries of these into their own fragment orders.  (Forming the entries inside the pack kernels -
// one 64-term fp64 chain per fragment element, on 64 workgroups - took 142 us per flow step; a training step at a batch of 256
// packs 8 flow steps per update.)
template <int DIM, int HEAD> struct VitFuse {
    static constexpr int LAYER_FLOATS = 2 * DIM * DIM + 2 * DIM;                     // scratch per layer
    static constexpr int M1 = 0, C1 = DIM * DIM, M2 = C1 + DIM, C2 = M2 + DIM * DIM;
};

// grid (depth, 2, FUSE_SPLIT): blocks (l, 0, *) form M1 / c1 of layer l, blocks (l, 1, *) M2 / c2, each a row range.  Both factors
// go through LDS first (coalesced loads; the 64-term fp64 chains then read LDS: straight from global memory, on 12 workgroups, the
// kernel took 98 us - more than the backward kernel of a flow step at a batch of 256).  `layers` = the flat parameters at layer 0.
constexpr int FUSE_SPLIT = 4;
struct VitFuseBatch {                                          // per flow step of a batch: its layers' flat parameters, its scratch
    const float* layers[kVitPrepBatch];
    float* scratch[kVitPrepBatch];
};
// blockIdx.x = layer + depth * (flow step of the batch)
template <int DIM, int HEAD>
__global__ __launch_bounds__(256) void k_vit_fuse(const VitFuseBatch fb, int depth) {
    using F = VitFuse<DIM, HEAD>;
    constexpr VitFlat P(0, DIM, HEAD);                        // (the per-layer offsets do not depend on the patch width)
    constexpr int GA = P.ga(), BA = P.ba(), WQ = P.wq(), WK = P.wk(), WV = P.wv(), WO = P.wo(), STRIDE = P.layer_stride();
    __shared__ float sA[HEAD * DIM], sB[HEAD * DIM];          // out[r][b] = sum_h sA[h][r] sB[h][b]
    __shared__ double tb[HEAD];
    const int bi = blockIdx.x / depth, layer = blockIdx.x - bi * depth;
    const float* p = fb.layers[bi] + (size_t)layer * STRIDE;
    float* out = fb.scratch[bi] + (size_t)layer * F::LAYER_FLOATS;
    const float *ga = p + GA, *ba = p + BA;
    const bool scores = blockIdx.y == 0;
    for (int i = threadIdx.x; i < HEAD * DIM; i += 256) {
        const int h = i / DIM, k = i - h * DIM;
        sA[i] = scores ? p[WK + i] : p[WO + k * HEAD + h];                    // Wk[h][r]  |  Wout[r][h] transposed
        sB[i] = scores ? p[WQ + i] : p[WV + i];                               // Wq[h][b]  |  Wv[h][b]
    }
    __syncthreads();
    if (threadIdx.x < HEAD) {                                  // Wq b (scores) or Wv b (value path), b = the norm's bias
        double a = 0.0;
        for (int k = 0; k < DIM; ++k) a += (double)sB[threadIdx.x * DIM + k] * (double)ba[k];
        tb[threadIdx.x] = a;
    }
    __syncthreads();
    constexpr int RPB = (DIM + FUSE_SPLIT - 1) / FUSE_SPLIT;   // rows per block
    const int r0 = blockIdx.z * RPB, r1 = min(DIM, r0 + RPB);
    for (int i = threadIdx.x; i < (r1 - r0) * (DIM + 1); i += 256) {
        const int r = r0 + i / (DIM + 1), b = i % (DIM + 1);   // consecutive threads: consecutive b (conflict-free sB rows); b == DIM: the bias entry
        double s = 0.0;
        if (b < DIM) {
#pragma unroll 8
            for (int h = 0; h < HEAD; ++h) s += (double)sA[h * DIM + r] * (double)sB[h * DIM + b];
            if (scores) out[F::M1 + r * DIM + b] = (float)(0.125 * s * (double)ga[r] * (double)ga[b]);
            else out[F::M2 + r * DIM + b] = (float)(s * (double)ga[b]);
        } else {
#pragma unroll 8
            for (int h = 0; h < HEAD; ++h) s += (double)sA[h * DIM + r] * tb[h];
            if (scores) out[F::C1 + r] = (float)(0.125 * s * (double)ga[r]);
            else out[F::C2 + r] = (float)s;
        }
    }
}

}  // namespace
