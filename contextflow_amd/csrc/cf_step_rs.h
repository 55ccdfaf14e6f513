// The two forward step families for small batches, whose waves split the output rows: k_flow_step_rs (8x8 and 4x4 levels) and
// k_flow_step_rs16 (4x4 level, one sample per workgroup), each with its chain form and launch helpers.  Included by cf_step.hip,
// which holds the launch lists that instantiate them; everything lives in an anonymous namespace of the including translation unit.
#pragma once
#include "cf_step_fwd.h"

namespace {

// ---- row-split forward step for SMALL batches (C = 32 on 8x8, C = 64 on 4x4) -------------------------------------------
// At the reference's batch sizes (64 / 256, config.py:10) a launch has far fewer workgroups than the chip has CUs, and
// the time of a step is the serial work of ONE workgroup: in k_flow_step a wave runs every row tile of its own pixel
// columns (C = 64: 4 tiles x 576 k-steps in the 3x3 alone).  Here the 4 waves of a workgroup share PIXR = 32 NPT pixel
// columns (2 samples at 4x4, 1 sample at 8x8) and split the OUTPUT ROWS: in phases 1 and 2 each wave owns one
// (row tile, pixel tile) pair, in phase 3 the two halves of K go to two waves whose partial sums meet in the epilogue.
// 4x the workgroups, a quarter of the serial MFMA chain per workgroup; the planes are exchanged through LDS with a
// workgroup barrier per phase.  Same packed workspace as k_flow_step.  Used below ~2 workgroups per CU (cf_flow_step_fwd).
// DUMP (training at small batches): the tape of cf_flow_step_fwd_taped - y0 / h1 / h2 planes, log-scale and y1, the ReLU
// mask words of this wave's (row tile, pixel tile) pairs, in the layout k_flow_step writes.
// KS = 2 (round 3): eight waves - waves 4..7 take the second half of the input channels of every tap of the 3x3, their
// partial sums meet waves 0..3's through the (then idle) T region.  What it buys is a second wave per SIMD to cover the
// first one's waits (35.0 -> 32.3 us at C = 64, 20.1 -> 19.1 at C = 32, batch of 256), NOT a shorter chain: the 2 304 MFMAs of a
// workgroup's 3x3 share the four matrix pipes of ONE CU whoever issues them (tools/dev/rs_ticks.py: phase 2 = 45.6 K of the
// 65 K cycles of a C = 64 step against 36.9 K of pure MFMA time).  Going below that needs more CUs per sample, i.e. 16-column
// tiles (one sample per workgroup at 4x4).
// timing-only probe build (tools/dev/make_abl.py ticks -DCF_RS_TICKS; read with tools/dev/rs_ticks.py): workgroup 0 leaves the
// cycles between the phase boundaries of k_flow_step_rs in z[wave * 16 + k] (the results of that build are garbage)
#ifdef CF_RS_TICKS
#define RS_TICK_INIT long long tacc_[12]; for (int k_ = 0; k_ < 12; ++k_) tacc_[k_] = 0; long long tprev_ = __builtin_readcyclecounter();
#define RS_TICK(k) { const long long tn_ = __builtin_readcyclecounter(); tacc_[k] += tn_ - tprev_; tprev_ = tn_; }
#define RS_TICK_DUMP if (blockIdx.x == 0 && lane == 0) for (int k_ = 0; k_ < 12; ++k_) z[wave * 16 + k_] = (float)tacc_[k_];
#else
#define RS_TICK_INIT
#define RS_TICK(k)
#define RS_TICK_DUMP
#endif
template <class G, int NPT, bool SQ, bool DUMP = false, int KS = 2>
__device__ __forceinline__ void flow_step_rs_body(const float* x, float* z, float* __restrict__ ldj_acc, const float* __restrict__ ws, int B,
                                                  int64_t xbs, StepTape tp = kNoTape) {
    constexpr int C = G::C, HW = G::HW, W = G::W, H = G::H, HALF = G::HALF, HID = G::HID, HP = G::HP;
    constexpr int PIXR = 32 * NPT, SPWR = PIXR / HW, RT1 = G::RT1, RT03 = G::RT03;
    static_assert(RT1 * NPT == 4 && RT03 * NPT == 2 && HP == HALF && PIXR % HW == 0, "row-split geometry");
    __shared__ __align__(16) float lds[(2 * C + HID + 2 * C) * PIXR];
    float* XP = lds;                         // [C][PIXR]    x plane
    float* Y = XP + C * PIXR;                // [C][PIXR]    rows [0, HALF) = y0, [HALF, C) = y1
    float* H1 = Y + C * PIXR;                // [HID][PIXR]  h1, then h2 in place
    float* T = H1 + HID * PIXR;              // [2][C][PIXR] the two K-halves of [t | raw]
    static_assert(KS == 2, "eight waves: the only form that is instantiated and tested");
    constexpr int NTH = 256 * KS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, lk = lane >> 5;
    const int w4 = wave & 3, kh2 = wave >> 2;          // phase 2: (row tile, pixel tile) pair of waves w4 and w4 + 4, channel half
    const int b0 = blockIdx.x * SPWR;
    const ws_rsrc_t rs = ws_rsrc(ws, G::WS_FLOATS);
    RS_TICK_INIT
    // the weight fragments of the three small products, requested before anything else (same reason as the ring of phase 2)
    const int rt1_ = (wave & 3) % RT1, it3_ = wave & 1, kh3_ = (wave >> 1) & 1, rt3_ = it3_ % RT03;
    constexpr int NGH3 = G::NG3 / 2;
    float4 f0[G::NG0], f1[G::NG1], f3[NGH3];
    if (wave < 2) {
#pragma unroll
        for (int g = 0; g < G::NG0; ++g) f0[g] = ws_frag(rs, lane, G::OFF_A0 + (g * RT03 + wave % RT03) * 256);
    }
    if (wave < 4) {
#pragma unroll
        for (int g = 0; g < G::NG1; ++g) f1[g] = ws_frag(rs, lane, G::OFF_A1 + (g * RT1 + rt1_) * 256);
#pragma unroll
        for (int g = 0; g < NGH3; ++g) f3[g] = ws_frag(rs, lane, G::OFF_A3 + ((kh3_ * NGH3 + g) * RT03 + rt3_) * 256);
    }
    __builtin_amdgcn_sched_barrier(0);

    // ---- x -> LDS (element-wise: small batches are not bandwidth-bound; Squeeze folded into the index)
#pragma unroll
    for (int i = 0; i < C * PIXR / NTH; ++i) {
        const int e = tid + NTH * i, ch = e / PIXR, col = e - ch * PIXR, sm = col / HW, pp = col - sm * HW;
        const int64_t bb = min(b0 + sm, B - 1);
        int src;
        if constexpr (!SQ) src = ch * HW + pp;
        else { const int yy = pp / W, xx = pp - yy * W; src = (ch >> 2) * 4 * HW + (2 * yy + ((ch >> 1) & 1)) * 2 * W + 2 * xx + (ch & 1); }
        XP[e] = x[bb * xbs + src];
    }
    __syncthreads();
    RS_TICK(0)
    // ---- phase 0: [y0 | y1] = W' x + b'   (waves 0, 1: one (row tile, pixel tile) pair each)
    if (wave < 2) {
        const int rt = wave % RT03, q = wave / RT03, col = q * 32 + li;
        f32x16 acc = bias_tile(ws + G::OFF_B0 + rt * 32, lk);
#pragma unroll
        for (int g = 0; g < G::NG0; ++g) {
            const float4 a = f0[g];
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (4 * g + e < G::KS0)
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(f4e(a, e), XP[(2 * (4 * g + e) + lk) * PIXR + col], acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) Y[(rt * 32 + tile_row(r, lk)) * PIXR + col] = acc[r];
    }
    __syncthreads();
    RS_TICK(1)
    // first half of the output = y0 (coupling.py:65)
#pragma unroll
    for (int i = 0; i < HALF * PIXR / NTH; ++i) {
        const int e = tid + NTH * i, ch = e / PIXR, col = e - ch * PIXR, sm = col / HW, pp = col - sm * HW;
        if (b0 + sm < B) {
            z[(int64_t)(b0 + sm) * C * HW + ch * HW + pp] = Y[e];
            if constexpr (DUMP) tp.y0[((int64_t)(b0 + sm) * HALF + ch) * HW + pp] = Y[e];
        }
    }
    const int rt1 = w4 % RT1, q1 = w4 / RT1, col1 = q1 * 32 + li;              // this wave's pair in phases 1, 2
    // tape helpers: the mask word of this wave's accumulator tile (global 32-column tile = blockIdx NPT + q1), and a
    // cooperative copy of the [HID][PIXR] plane in LDS to its (B, HID, HW) place
    auto mask_word = [&](unsigned* __restrict__ m, const f32x16& a) {
        unsigned bits = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) bits |= (a[r] > 0.f ? 1u : 0u) << r;
        m[((int64_t)(blockIdx.x * NPT + q1) * RT1 + rt1) * 64 + lane] = bits;
    };
    auto plane_dump = [&](float* __restrict__ dst) {
#pragma unroll
        for (int i = 0; i < HID * PIXR / NTH; ++i) {
            const int e = tid + NTH * i, ch = e / PIXR, col = e - ch * PIXR, sm = col / HW, pp = col - sm * HW;
            if (b0 + sm < B) dst[((int64_t)(b0 + sm) * HID + ch) * HW + pp] = H1[e];
        }
    };
    RS_TICK(2)
    // ---- phase 1: h1 = relu(NN.0 y0 + b)
    if (wave < 4) {
        f32x16 acc = bias_tile(ws + G::OFF_B1 + rt1 * 32, lk);
#pragma unroll
        for (int g = 0; g < G::NG1; ++g) {
            const float4 a = f1[g];
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (4 * g + e < G::KS1)
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(f4e(a, e), Y[(2 * (4 * g + e) + lk) * PIXR + col1], acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) H1[(rt1 * 32 + tile_row(r, lk)) * PIXR + col1] = cf_relu(acc[r]);
        if constexpr (DUMP) mask_word(tp.m1, acc);
    }
    __syncthreads();
    RS_TICK(3)
    if constexpr (DUMP) plane_dump(tp.h1);
    // ---- phase 2: h2 = relu(NN.2 (*) h1 + b), 3x3 reflect: K = 9 taps x HID channels, fragments one group ahead
    f32x16 acc2 = bias_tile(ws + G::OFF_B2 + rt1 * 32, lk);
    if (kh2) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc2[r] = 0.f;
    }
    {
        const int sm = col1 / HW, pp = col1 - sm * HW, py = pp / W, px = pp - py * W;
        // a wave has ONE row tile here: 4 MFMAs (256 cycles) per weight fragment, less than an L2 round trip under load -
        // the fragments run in a ring of 4, fetched three groups ahead.  This wave's sequence of groups: for every tap the NH
        // channel groups of its half, cg0 .. cg0 + NH - 1
        constexpr int NH = G::NCG / KS;
        // ring depth: at a batch of 256 the packed weights of a step (0.16-0.66 MB, 6 MB over the twelve steps of a forward)
        // come from the Infinity Cache, not from L2 - measured ~1900 cycles per fragment under the load of 128 workgroups
        // streaming the same 590 KB (tools/dev/rs_ticks.py: 634 cycles per 256-cycle MFMA group with three loads in
        // flight).  Seven in flight cover it.
        constexpr int RD = NH % 8 == 0 ? 8 : 4;
        static_assert(NH % RD == 0, "fragment ring");
        const int cg0 = kh2 * NH;
        auto seq_frag = [&](int tap, int c) {              // fragment offset of group (tap, cg0 + c); c may run past NH into the next tap
            const int t2 = tap + c / NH, c2 = c % NH;
            const int g = (t2 < 9 ? t2 : 8) * G::NCG + cg0 + (t2 < 9 ? c2 : NH - 1);
            return G::OFF_A2 + (g * RT1 + rt1) * 256;
        };
        float4 a[RD];
#pragma unroll
        for (int j = 0; j < RD - 1; ++j) a[j] = ws_frag(rs, lane, seq_frag(0, j));
        // ... and the B operands (LDS) one group ahead: with a single accumulator chain per wave nothing else hides the
        // LDS latency in front of each group's first MFMA
        auto tap_src = [&](int tap) -> const float* {
            int yy = py + tap / 3 - 1, xx = px + tap % 3 - 1;
            yy = yy < 0 ? -yy : (yy >= H ? 2 * (H - 1) - yy : yy);
            xx = xx < 0 ? -xx : (xx >= W ? 2 * (W - 1) - xx : xx);
            return H1 + sm * HW + yy * W + xx + (lk + 8 * cg0) * PIXR;      // channel 8 cg0 + lk of the source pixel
        };
        float bv[2][4];
        const float* src = tap_src(0);
#pragma unroll
        for (int e = 0; e < 4; ++e) bv[0][e] = src[2 * e * PIXR];
#pragma unroll 1
        for (int tap = 0; tap < 9; ++tap) {
            const float* nsrc = tap_src(tap < 8 ? tap + 1 : 8);
#pragma unroll
            for (int c = 0; c < NH; ++c) {
                a[(c + RD - 1) & (RD - 1)] = ws_frag(rs, lane, seq_frag(tap, c + RD - 1));
#pragma unroll
                for (int e = 0; e < 4; ++e)       // next group: same tap, next 8 channels - or the first 8 of the next tap
                    bv[(c + 1) & 1][e] = (c + 1 < NH) ? src[(8 * (c + 1) + 2 * e) * PIXR] : nsrc[2 * e * PIXR];
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(f4e(a[c & (RD - 1)], e), bv[c & 1][e], acc2, 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
            src = nsrc;
        }
    }
    RS_TICK(4)
    __syncthreads();                 // every wave has finished reading h1
    RS_TICK(5)
    if constexpr (KS > 1) {          // the two channel halves meet (T is idle until phase 3)
        if (kh2) {
#pragma unroll
            for (int r = 0; r < 16; ++r) T[(rt1 * 32 + tile_row(r, lk)) * PIXR + col1] = acc2[r];
        }
        __syncthreads();
        if (!kh2) {
#pragma unroll
            for (int r = 0; r < 16; ++r) acc2[r] += T[(rt1 * 32 + tile_row(r, lk)) * PIXR + col1];
        }
    }
    if (!kh2) {
#pragma unroll
        for (int r = 0; r < 16; ++r) H1[(rt1 * 32 + tile_row(r, lk)) * PIXR + col1] = cf_relu(acc2[r]);
        if constexpr (DUMP) mask_word(tp.m2, acc2);
    }
    __syncthreads();
    RS_TICK(6)
    if constexpr (DUMP) plane_dump(tp.h2);
    // ---- phase 3: [t | raw] = NN.4 h2 + b: pair = wave & 1, K half = wave >> 1 (the bias rides with half 0)
    if (wave < 4) {
        const int it = wave & 1, kh = wave >> 1, rt = it % RT03, q = it / RT03, col = q * 32 + li;
        f32x16 acc = bias_tile(ws + G::OFF_B3 + rt * 32, lk);
        if (kh) {
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        }
        constexpr int NGH = G::NG3 / 2;
        static_assert(G::NG3 % 2 == 0 && G::KS3 % 8 == 0, "phase-3 K halves");
#pragma unroll
        for (int gg = 0; gg < NGH; ++gg) {
            const int g = kh * NGH + gg;
            const float4 a = f3[gg];
#pragma unroll
            for (int e = 0; e < 4; ++e)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(f4e(a, e), H1[(2 * (4 * g + e) + lk) * PIXR + col], acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) T[(kh * C + rt * 32 + tile_row(r, lk)) * PIXR + col] = acc[r];
    }
    __syncthreads();
    RS_TICK(7)
    // ---- affine map and log-det over the first 256 threads: element e = (channel, column); a thread's column is fixed
    float lsum = 0.f;
    if (wave < 4) {
    const int colE = tid % PIXR, smE = colE / HW, ppE = colE - smE * HW;
#pragma unroll
    for (int i = 0; i < HALF * PIXR / 256; ++i) {
        const int ch = (tid + 256 * i) / PIXR;
        const float tt = T[ch * PIXR + colE] + T[(C + ch) * PIXR + colE];
        const float raw = T[(HP + ch) * PIXR + colE] + T[(C + HP + ch) * PIXR + colE];
        const float ls = cf_log_scale(raw);
        const float y1v = Y[(HP + ch) * PIXR + colE];
        const float z1 = fmaf(y1v, __expf(ls), tt);
        lsum += ls;
        if (b0 + smE < B) {
            z[(int64_t)(b0 + smE) * C * HW + (HALF + ch) * HW + ppE] = z1;
            if constexpr (DUMP) {
                const int64_t o = ((int64_t)(b0 + smE) * HALF + ch) * HW + ppE;
                tp.ls[o] = ls;
                tp.y1[o] = y1v;
            }
        }
    }
    // per-sample sum: the lanes of a sample inside the wave (columns are lane % PIXR), then across the waves through LDS
    constexpr int LPS = HW < 64 ? HW : 64;            // consecutive lanes of one sample
#pragma unroll
    for (int o = 1; o < LPS; o <<= 1) lsum += __shfl_xor(lsum, o, 64);
    if (PIXR < 64 && HW < 32) lsum += __shfl_xor(lsum, 32, 64);    // PIXR = 32: lanes l and l + 32 hold the same column
    }
    __syncthreads();                                  // T is dead: reuse its first words
    constexpr int LPS2 = HW < 64 ? HW : 64;
    if (wave < 4 && (lane % LPS2) == 0 && (PIXR >= 64 || lane < 32)) T[wave * 4 + (lane % PIXR) / HW] = lsum;
    __syncthreads();
    if (tid < SPWR && b0 + tid < B) ldj_acc[b0 + tid] += ws[0] + ((T[tid] + T[4 + tid]) + (T[8 + tid] + T[12 + tid]));
    RS_TICK(8)
    RS_TICK_DUMP
}

template <class G, int NPT, bool SQ, bool DUMP = false, int KS = 2>
__global__ __launch_bounds__(256 * KS) void k_flow_step_rs(const float* __restrict__ x, float* __restrict__ z,
                                                      float* __restrict__ ldj_acc, const float* __restrict__ ws, int B,
                                                      int64_t xbs, StepTape tp = kNoTape) {
    flow_step_rs_body<G, NPT, SQ, DUMP, KS>(x, z, ldj_acc, ws, B, xbs, tp);
}
template <class G, int NPT, bool SQ, int KS = 2>
__global__ __launch_bounds__(256 * KS) void k_flow_step_rs_chain(const float* x, float* z, float* __restrict__ ldj_acc, const WsChain wc,
                                                            int nsteps, int B, int64_t xbs) {
    flow_step_rs_body<G, NPT, SQ, false, KS>(x, z, ldj_acc, wc.ws[0], B, xbs);
    for (int st = 1; st < nsteps; ++st) {
        __syncthreads();
        flow_step_rs_body<G, NPT, false, false, KS>(z, z, ldj_acc, wc.ws[st], B, (int64_t)G::C * G::HW);
    }
}
template <class G, int NPT>
int launch_step_rs_chain(const StepArgs& a, const WsChain& wc, int n) {
    constexpr int SPWR = 32 * NPT / G::HW;
    const auto k = a.sq ? k_flow_step_rs_chain<G, NPT, true, 2> : k_flow_step_rs_chain<G, NPT, false, 2>;
    k<<<dim3((a.B + SPWR - 1) / SPWR), dim3(512), 0, a.s>>>(a.x, a.z, a.ldj, wc, n, a.B, a.xbs);
    return 0;
}

template <class G, int NPT, bool DUMP = false>
int launch_step_rs(const StepArgs& a) {
    constexpr int SPWR = 32 * NPT / G::HW;
    constexpr int KS = 2;
    const auto k = a.sq ? k_flow_step_rs<G, NPT, true, DUMP, KS> : k_flow_step_rs<G, NPT, false, DUMP, KS>;
    k<<<dim3((a.B + SPWR - 1) / SPWR), dim3(256 * KS), 0, a.s>>>(a.x, a.z, a.ldj, a.ws, a.B, a.xbs, a.tp);
    return 0;
}

// ---- the 4x4 level at small batches: ONE sample per workgroup on 16-column tiles -------------------------------------------
// tools/dev/rs_ticks.py: at a batch of 256 the row-split kernel above spends 45.6 K of its 65 K cycles in the 3x3 - against
// 36.9 K of pure MFMA time: the 2 304 MFMAs of a workgroup's 3x3 (2 samples = 32 pixel columns of a 32x32x2 tile) share the
// four matrix pipes of ONE CU, and the launch has 128 workgroups for 256 CUs.  v_mfma_f32_16x16x4_f32 tiles hold exactly one
// 4x4 sample in their 16 columns: twice the workgroups, half the matrix work each.  The four waves split the output rows
// (16-row tiles: 1 / 2 / 2 / 1 per wave in the four products), planes [channel][16 pixels] in LDS (20 KB), natural row
// order (t / raw / y1 of a channel meet in the LDS epilogue), the fragments of the three small products requested at
// kernel start, those of the 3x3 through a ring of four groups.
// DUMP (training): the tape of cf_flow_step_fwd_taped - the planes are the LDS planes themselves (whole 16-byte rows), a mask
// word of the 32x32x2 layout is put together from the four 4-bit groups two lanes (g, g + 2) hold of it.
template <class G, bool SQ, bool DUMP = false>
__device__ __forceinline__ void flow_step_rs16_body(const float* x, float* z, float* __restrict__ ldj_acc, const float* __restrict__ ws, int B,
                                                    int64_t xbs, StepTape tp = kNoTape) {
    static_assert(G::RS16, "C = 64 on 4x4 images");
    constexpr int C = G::C, HW = 16, W = 4, H = 4, HALF = G::HALF, HID = G::HID, P = 16;
    constexpr int NG0 = C / 16, NG1 = HALF / 16, NGT = HID / 16, NG3 = HID / 16;            // groups of 4 k-steps: per product / per tap
    __shared__ __align__(16) float lds[(C + C + HID + C) * P + 4];
    float* XP = lds;                 // [C][16]    x
    float* YP = XP + C * P;          // [C][16]    y0 | y1
    float* H1 = YP + C * P;          // [HID][16]  h1, then h2 in place
    float* TP = H1 + HID * P;        // [C][16]    t | raw
    float* red = TP + C * P;         // [4]
    const int tid = threadIdx.x, lane = tid & 63, col = lane & 15, g = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.x;
    const ws_rsrc_t rs = ws_rsrc(ws, G::WS_FLOATS);
    float4 f0[NG0], f1[2][NG1], f3[NG3];
#pragma unroll
    for (int gi = 0; gi < NG0; ++gi) f0[gi] = ws_frag(rs, lane, G::OFF_RA0 + (w * NG0 + gi) * 256);
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int gi = 0; gi < NG1; ++gi) f1[t][gi] = ws_frag(rs, lane, G::OFF_RA1 + ((2 * w + t) * NG1 + gi) * 256);
#pragma unroll
    for (int gi = 0; gi < NG3; ++gi) f3[gi] = ws_frag(rs, lane, G::OFF_RA3 + (w * NG3 + gi) * 256);
    // the 3x3: group sequence j = tap * NGT + channel group, two row tiles per group, ring of four groups
    auto frag2 = [&](int j, float4 (&o)[2]) {
        const int jj = j < 9 * NGT ? j : 9 * NGT - 1;
#pragma unroll
        for (int t = 0; t < 2; ++t) o[t] = ws_frag(rs, lane, G::OFF_RA2 + ((2 * w + t) * 9 * NGT + jj) * 256);
    };
    float4 ring[4][2];
#pragma unroll
    for (int j = 0; j < 3; ++j) frag2(j, ring[j]);
    __builtin_amdgcn_sched_barrier(0);
    const float* xb = x + (int64_t)b * xbs;
#pragma unroll
    for (int i = 0; i < C * P / 256; ++i) {
        const int e = tid + 256 * i, ch = e / P, pp = e - ch * P;
        int src;
        if constexpr (!SQ) src = ch * HW + pp;
        else { const int yy = pp / W, xx = pp - yy * W; src = (ch >> 2) * 4 * HW + (2 * yy + ((ch >> 1) & 1)) * 2 * W + 2 * xx + (ch & 1); }
        XP[e] = xb[src];
    }
    __syncthreads();
    auto mma = [](float a, float bv, f32x4 acc) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv, acc, 0, 0, 0); };
    auto bias4 = [&](int off, int rt) {
        const float4 v = *reinterpret_cast<const float4*>(ws + off + 16 * rt + 4 * g);
        return f32x4{v.x, v.y, v.z, v.w};
    };
    // ---- phase 0: [y0 | y1] = e^{-logs} (Wm x - t), rows 16 w ..
    {
        f32x4 a0 = bias4(G::OFF_RB0, w), a1 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 4 * NG0; ++s) {
            const float bv = XP[(4 * s + g) * P + col];
            if (s & 1) a1 = mma(f4e(f0[s >> 2], s & 3), bv, a1); else a0 = mma(f4e(f0[s >> 2], s & 3), bv, a0);
        }
        a0 += a1;
#pragma unroll
        for (int r = 0; r < 4; ++r) YP[(16 * w + 4 * g + r) * P + col] = a0[r];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < HALF * P / 256; ++i) {                                 // first half of the output = y0 (coupling.py:65)
        const int e = tid + 256 * i;
        z[(int64_t)b * C * HW + e] = YP[e];
        if constexpr (DUMP) tp.y0[(int64_t)b * HALF * HW + e] = YP[e];
    }
    // tape helpers: this lane's bits of the mask word of 32-row tile w (rows 16 t + 4 g + r -> bit 4 (2 t + g / 2) + r of the
    // word of lane (g & 1) * 32 + column), and the copy of a [HID][16] plane to its (B, HID, 16) place
    auto mask_word = [&](unsigned* __restrict__ m, const f32x4 (&a)[2]) {
        unsigned bits = 0;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) bits |= (a[t][r] > 0.f ? 1u : 0u) << (4 * (2 * t + (g >> 1)) + r);
        bits |= (unsigned)__shfl_xor((int)bits, 32);
        if (g < 2) m[((int64_t)(b >> 1) * G::RT1 + w) * 64 + g * 32 + (b & 1) * 16 + col] = bits;
    };
    auto plane_dump = [&](float* __restrict__ dst) {
        for (int e = 4 * tid; e < HID * P; e += 1024)
            *reinterpret_cast<float4*>(dst + (int64_t)b * HID * HW + e) = *reinterpret_cast<const float4*>(H1 + e);
    };
    // ---- phase 1: h1 = relu(NN.0 y0 + b), row tiles 2 w, 2 w + 1
    {
        f32x4 a[2] = {bias4(G::OFF_RB1, 2 * w), bias4(G::OFF_RB1, 2 * w + 1)};
#pragma unroll
        for (int s = 0; s < 4 * NG1; ++s) {
            const float bv = YP[(4 * s + g) * P + col];
#pragma unroll
            for (int t = 0; t < 2; ++t) a[t] = mma(f4e(f1[t][s >> 2], s & 3), bv, a[t]);
        }
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) H1[(16 * (2 * w + t) + 4 * g + r) * P + col] = cf_relu(a[t][r]);
        if constexpr (DUMP) mask_word(tp.m1, a);
    }
    __syncthreads();
    if constexpr (DUMP) plane_dump(tp.h1);
    // ---- phase 2: h2 = relu(NN.2 (*) h1 + b), 3x3 with reflect padding: 9 taps x HID channels
    f32x4 a2[2] = {bias4(G::OFF_RB2, 2 * w), bias4(G::OFF_RB2, 2 * w + 1)};
    {
        const int py = col / W, px = col - py * W;
        auto tap_src = [&](int tap) {
            int yy = py + tap / 3 - 1, xx = px + tap % 3 - 1;
            yy = yy < 0 ? -yy : (yy >= H ? 2 * (H - 1) - yy : yy);
            xx = xx < 0 ? -xx : (xx >= W ? 2 * (W - 1) - xx : xx);
            return g * P + yy * W + xx;                                        // + 4 s P per k-step
        };
        float bv[2][4];
        int src = tap_src(0);
#pragma unroll
        for (int e = 0; e < 4; ++e) bv[0][e] = H1[src + 4 * e * P];
#pragma unroll 1
        for (int tap = 0; tap < 9; ++tap) {
            const int nsrc = tap_src(tap < 8 ? tap + 1 : 8);
#pragma unroll
            for (int c = 0; c < NGT; ++c) {                                    // NGT = 8: static ring slots
                frag2(tap * NGT + c + 3, ring[(c + 3) & 3]);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    bv[(c + 1) & 1][e] = (c + 1 < NGT) ? H1[src + (16 * (c + 1) + 4 * e) * P] : H1[nsrc + 4 * e * P];
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int t = 0; t < 2; ++t) a2[t] = mma(f4e(ring[c & 3][t], e), bv[c & 1][e], a2[t]);
                __builtin_amdgcn_sched_barrier(0);
            }
            src = nsrc;
        }
    }
    __syncthreads();                 // every wave has finished reading h1
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) H1[(16 * (2 * w + t) + 4 * g + r) * P + col] = cf_relu(a2[t][r]);
    if constexpr (DUMP) mask_word(tp.m2, a2);
    __syncthreads();
    if constexpr (DUMP) plane_dump(tp.h2);
    // ---- phase 3: [t | raw] = NN.4 h2 + b, rows 16 w ..
    {
        f32x4 a0 = bias4(G::OFF_RB3, w), a1 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 4 * NG3; ++s) {
            const float bv = H1[(4 * s + g) * P + col];
            if (s & 1) a1 = mma(f4e(f3[s >> 2], s & 3), bv, a1); else a0 = mma(f4e(f3[s >> 2], s & 3), bv, a0);
        }
        a0 += a1;
#pragma unroll
        for (int r = 0; r < 4; ++r) TP[(16 * w + 4 * g + r) * P + col] = a0[r];
    }
    __syncthreads();
    // ---- affine map and log-det (coupling.py:52-66): element (channel, pixel), two per thread
    float lsum = 0.f;
#pragma unroll
    for (int i = 0; i < HALF * P / 256; ++i) {
        const int e = tid + 256 * i;
        const float ls = cf_log_scale(TP[HALF * P + e]);
        z[(int64_t)b * C * HW + HALF * HW + e] = fmaf(YP[HALF * P + e], __expf(ls), TP[e]);
        if constexpr (DUMP) { tp.ls[(int64_t)b * HALF * HW + e] = ls; tp.y1[(int64_t)b * HALF * HW + e] = YP[HALF * P + e]; }
        lsum += ls;
    }
    lsum = cf_block_sum<4>(lsum, red);
    if (tid == 0) ldj_acc[b] += ws[0] + lsum;
}
template <class G, bool SQ, bool DUMP = false>
__global__ __launch_bounds__(256) void k_flow_step_rs16(const float* __restrict__ x, float* __restrict__ z,
                                                        float* __restrict__ ldj_acc, const float* __restrict__ ws, int B,
                                                        int64_t xbs, StepTape tp) {
    flow_step_rs16_body<G, SQ, DUMP>(x, z, ldj_acc, ws, B, xbs, tp);
}
template <class G, bool SQ>
__global__ __launch_bounds__(256) void k_flow_step_rs16_chain(const float* x, float* z, float* __restrict__ ldj_acc, const WsChain wc,
                                                              int nsteps, int B, int64_t xbs) {
    flow_step_rs16_body<G, SQ>(x, z, ldj_acc, wc.ws[0], B, xbs);
    for (int st = 1; st < nsteps; ++st) {
        __syncthreads();
        flow_step_rs16_body<G, false>(z, z, ldj_acc, wc.ws[st], B, (int64_t)G::C * G::HW);
    }
}
template <class G>
int launch_step_rs16_chain(const StepArgs& a, const WsChain& wc, int n) {
    const auto k = a.sq ? k_flow_step_rs16_chain<G, true> : k_flow_step_rs16_chain<G, false>;
    k<<<dim3(a.B), dim3(256), 0, a.s>>>(a.x, a.z, a.ldj, wc, n, a.B, a.xbs);
    return 0;
}
template <class G, bool DUMP = false>
int launch_step_rs16(const StepArgs& a) {
    const auto k = a.sq ? k_flow_step_rs16<G, true, DUMP> : k_flow_step_rs16<G, false, DUMP>;
    k<<<dim3(a.B), dim3(256), 0, a.s>>>(a.x, a.z, a.ldj, a.ws, a.B, a.xbs, a.tp);
    return 0;
}

}  // namespace
