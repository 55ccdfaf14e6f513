// The forward step of the 16x16 level (C = 8 / 16), one sample per workgroup on 16x16x4 tiles: flow_step_small_phases,
// flow_step_small_body, k_flow_step_small with its chain and level forms and their launch helpers.  Included by cf_step.hip, which
// holds the launch lists that instantiate them; everything lives in an anonymous namespace of the including translation unit.
#pragma once
#include "cf_step_fwd.h"

namespace {

// ---- small-channel forward step (C = 8 / 16 on 16x16 images: first resolution level of mnist / cifar10) ------------
// Same data flow as k_flow_step, one sample per workgroup, but the phases with <= 16 output rows run on
// v_mfma_f32_16x16x4_f32 tiles (same flop/cycle as 32x32x2, no padding rows):
//   phase 0  [y0 | y1] = W'x + b'   16 packed rows (chan_of_row16)                        K = C
//   phase 1  h1 = relu(NN.0 y0)     C = 16: 32 rows on 32x32x2 (conditioner_net);  C = 8: 16 rows on 16x16x4
//   phase 2  3x3 reflect conv       C = 16: 32x32x2, taps unrolled;                 C = 8: 16x16x4, a column tile is one
//                                   image row, so the reflected source row of a tap is a scalar
//   phase 3  [t | raw] = NN.4 h2    16 packed rows                                        K = 2C
// Result tile of the 16x16x4 form: column (pixel) = lane & 15, rows 4 (lane >> 4) + r in the 4 registers; the packing
// puts t, raw and y1 of channels 2g, 2g+1 into lane group g, so the affine epilogue is lane-local again.
// In the 16-row phases lanes l and l + 16 read the same bank (rows k, k+1 of a [row][256] plane): a 2-way conflict on
// ~100 ds_read_b32 per wave, i.e. a few hundred LDS cycles against ~22 000 MFMA cycles.

// DUMP (training): y0 and the post-ReLU h1 / h2 planes also go to the tape `tp` (see k_flow_step).
// CF_G16W_MINW: waves per SIMD the C = 16 Winograd geometry is compiled for (A/B builds of tools/dev/make_abl.py)
#ifndef CF_G16W_MINW
#define CF_G16W_MINW 4
#endif
// CTX: per-sample bias of the specialist coupling (see conditioner_net): 1 sb (B, C) on the conditioner output, 2 sb (B, 2C)
// before the first ReLU.
// (x and z carry no __restrict__: the chained form below runs steps 2.. IN PLACE on the z of the step before)
// timing-only probe (-DCF_ABL_NOCONF): the B-operand reads of the 16-row phases without their bank conflict (rows 4s + lg of a
// 256-float plane share a bank): the lane group shifts the COLUMN instead - wrong data, conflict-free
#ifdef CF_ABL_NOCONF
#define CF_ROWIDX(r, lg) ((r) * PIX + ((lg) * 16 & 63))
#else
#define CF_ROWIDX(r, lg) (((r) + (lg)) * PIX)
#endif
// flow_step_small_phases: phases 0-3, the affine map and the log-det of ONE step on the x plane in rows [0, C) of H1 - the one body of
// the single-step kernel, of the small-batch chain and of the level kernel (k_flow_step_small_level).
// LEVEL: the step is one of a run that stays in LDS.  Nothing of z goes to global memory here; z = [y0 | z1] becomes the next step's
// x plane - y0 from the Y0 plane (every lane takes back its own words), z1 straight from the registers.  Cross-wave hazards of a step
// boundary: (1) the log-det scratch - four partial sums that thread 0 reads behind the step's last workgroup barrier - sits in row C
// of H1 instead of Y0: the next step's phase 0 writes Y0 at once, row C of H1 not before the barrier in front of its h1 writes, which
// thread 0 reaches with the sums read; (2) C = 8: the next step's Winograd-domain weights overwrite this step's in LDS - behind that
// same last barrier, which every wave reaches after its phase 2.  Everything else a wave touches between that barrier and the next
// step's first one is its own pixel columns.
template <class G, bool DBG, bool DUMP, int CTX, bool LEVEL>
__device__ __forceinline__ void flow_step_small_phases(float* z, float* __restrict__ ldj_acc, const float* __restrict__ ws, int B,
                                                       float* __restrict__ dbg, StepTape tp, const float* __restrict__ sb, int wave_u = 0) {
    static_assert(G::SMALL, "16x16 images, one sample per workgroup, C <= 16");
    static_assert(CTX == 0 || !G::HID16, "the per-sample bias is wired into the 32-row conditioner phases (C = 16)");
    static_assert(!LEVEL || (G::WINO && CTX == 0 && !DUMP && !DBG), "level form: the evaluation step in its Winograd geometry");
    constexpr int C = G::C, W = 16, H = 16, PIX = 256, HALF = G::HALF, HID = G::HID, PTW = G::PTW;
    extern __shared__ __align__(16) float lds[];
    float* Y0 = lds;                    // [HALF][PIX]
    float* H1 = lds + HALF * PIX;       // [HID][PIX]: x plane, then h1, then h2
    const int tid_ = LEVEL ? wave_u * 64 + cf_lane_fresh() : (int)threadIdx.x;      // (LEVEL: per step, see cf_lane_fresh)
    const int tid = tid_, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, lg = lane >> 4;
    const int tile = blockIdx.x;        // = sample index
    const int colb = wave * 64 + l15;   // this lane's pixel column in column tile 0 (tile ct: + 16 ct)

    const ws_rsrc_t rs = ws_rsrc(ws, G::WS_FLOATS);
    if constexpr (G::LDS_W > 0) {
        // the Winograd-domain weights of the 3x3 into LDS (16 KB, fragment order as packed): read by every wave of phase 2,
        // two workgroup barriers from here
        float* WL = lds + (HALF + HID) * PIX;
#pragma unroll
        for (int i = 0; i < G::LDS_W / 1024; ++i)
            *reinterpret_cast<float4*>(WL + (i * 256 + tid) * 4) = ws_frag(rs, tid, G::OFF_AW + i * 1024);
    }
    cf_wave_sync();

    // ================= phase 0: [y0 | y1] = (e^{-logs} Wm) x - t e^{-logs}   (conv1x1.py:54 + actnorm.py:59)
    f32x4 acc0[4];
    {
        const float4 b = *reinterpret_cast<const float4*>(ws + G::OFF_SB0 + 4 * lg);
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) { acc0[ct][0] = b.x; acc0[ct][1] = b.y; acc0[ct][2] = b.z; acc0[ct][3] = b.w; }
#pragma unroll
        for (int g = 0; g < G::SG0; ++g) {
            const float4 a = ws_frag(rs, lane, G::OFF_SA0 + g * 256);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (4 * (4 * g + e) < C) {
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct)
                        acc0[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(f4e(a, e), H1[CF_ROWIDX(4 * (4 * g + e), lg) + colb + 16 * ct],
                                                                        acc0[ct], 0, 0, 0);
                }
        }
    }
    // first half -> LDS (conditioner input and first half of the output, coupling.py:65); y1 stays in acc0[.][2..3]
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int j = 0; j < 2; ++j)
            if (2 * lg + j < HALF) Y0[(2 * lg + j) * PIX + colb + 16 * ct] = acc0[ct][j];
    if constexpr (LEVEL) {               // y1 is pinned here (see flow_step_phases)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) { asm volatile("" : "+v"(acc0[ct][2])); asm volatile("" : "+v"(acc0[ct][3])); }
    }
    cf_wave_sync();
    if constexpr (!LEVEL) z_store<G>(z, Y0, tile, 0, B, wave, lane);
    if constexpr (DUMP) rows_store_t<G, HALF, HALF>(tp.y0, Y0, tile, B, wave, lane);
    const int64_t dbg_cols = (int64_t)B * PIX;      // test-only dumps (DBG): planes as [rows][B * PIX], see k_flow_step
    auto dump = [&](const float* plane, int rows, int row0) {
        __syncthreads();
        for (int e = tid; e < rows * PIX; e += 256) dbg[(int64_t)(row0 + e / PIX) * dbg_cols + (int64_t)tile * PIX + (e % PIX)] = plane[e];
        __syncthreads();
    };
    if constexpr (DBG) dump(Y0, HALF, 0);
    // C = 8 (16 hidden rows on 16x16x4 tiles): the tape's ReLU mask words are defined in the 32x32x2 accumulator layout
    // (StepTape) - taken from the plane in LDS, this wave's own columns (rows_store_t before it ends with a wave fence)
    auto plane_mask_store = [&](unsigned* __restrict__ m) {
        const int li = lane & 31, lk = lane >> 5;
#pragma unroll
        for (int q = 0; q < PTW; ++q) {
            unsigned b = 0;
#pragma unroll
            for (int r = 0; r < 8; ++r) b |= (H1[tile_row(r, lk) * PIX + (wave * PTW + q) * 32 + li] > 0.f ? 1u : 0u) << r;
            m[((int64_t)tile * G::NPT + wave * PTW + q) * 64 + lane] = b;
        }
    };
    (void)plane_mask_store;

    // ================= phases 1, 2: h2 = relu(NN.2 (*) relu(NN.0 y0 + b) + b)   (coupling.py:26-27)
    if constexpr (!G::HID16) {
        const int li = lane & 31;
        int pix[PTW], pin[PTW];
#pragma unroll
        for (int q = 0; q < PTW; ++q) { pix[q] = (wave * PTW + q) * 32 + li; pin[q] = pix[q]; }
        f32x16 unused[G::RT03][PTW];
        int soff[PTW];
#pragma unroll
        for (int q = 0; q < PTW; ++q) soff[q] = tile * HID;
        conditioner_net<G, CTX == 2 ? 2 : 0, DUMP, 2>(unused, lds, ws, pix, pin, lane, tid, DBG ? dbg : nullptr, dbg_cols, tile,
                                                      CTX == 2 ? sb : nullptr, soff, tp, B);
    } else {
        f32x4 a1[4];
        {
            const float4 b = *reinterpret_cast<const float4*>(ws + G::OFF_B1 + 4 * lg);
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) { a1[ct][0] = b.x; a1[ct][1] = b.y; a1[ct][2] = b.z; a1[ct][3] = b.w; }
            const float4 a = ws_frag(rs, lane, G::OFF_SA1);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (4 * e < HALF) {
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct)
                        a1[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(f4e(a, e), Y0[(4 * e + lg) * PIX + colb + 16 * ct], a1[ct], 0, 0, 0);
                }
            if constexpr (G::WINO) {
                // Winograd form of the 3x3 (cf_step_common.h: winograd_phase2): h1 goes to LDS in its parity-split pixel
                // order, which scatters a wave's pixels over the whole sample - every wave must be done with the x plane
                static_assert(!DUMP && !DBG, "the tape / the dumps are written by the direct-form geometry");
                __syncthreads();
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) {
                    const int pw = wino_pix<G>(0, wave * 4 + ct, l15);      // a column tile is one image row
#pragma unroll
                    for (int r = 0; r < 4; ++r) H1[(4 * lg + r) * PIX + (pw ^ ((r & 1) * (W / 2)))] = cf_relu(a1[ct][r]);
                }
            } else {
#pragma unroll
                for (int ct = 0; ct < 4; ++ct)
#pragma unroll
                    for (int r = 0; r < 4; ++r) H1[(4 * lg + r) * PIX + colb + 16 * ct] = cf_relu(a1[ct][r]);
            }
            if constexpr (DUMP) { rows_store_t<G, HID, HID>(tp.h1, H1, tile, B, wave, lane); plane_mask_store(tp.m1); }
        }
        __syncthreads();                 // h1 complete: the 3x3 taps read neighbouring waves' image rows
        if constexpr (DBG) dump(H1, HID, C);
        if constexpr (G::WINO) {
            winograd_phase2<G>(lds, ws, rs, lane, wave);       // ends with h2 (ReLU, bias) in natural order, own columns
        } else {
        f32x4 a2[4];
        {
            const float4 b = *reinterpret_cast<const float4*>(ws + G::OFF_B2 + 4 * lg);
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) { a2[ct][0] = b.x; a2[ct][1] = b.y; a2[ct][2] = b.z; a2[ct][3] = b.w; }
            int xo[3];                   // reflected source column per dx, plus this lane's k row of the h1 plane
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                int xx = l15 + d - 1;
                xx = xx < 0 ? -xx : (xx >= W ? 2 * (W - 1) - xx : xx);
                xo[d] = HALF * PIX + lg * PIX + xx;
            }
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const float4 a = ws_frag(rs, lane, G::OFF_SA2 + tap * 256);
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) {
                    int yy = wave * 4 + ct + tap / 3 - 1;            // wave-uniform: a column tile is one image row
                    yy = yy < 0 ? -yy : (yy >= H ? 2 * (H - 1) - yy : yy);
                    const int src = xo[tap % 3] + yy * W;
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        a2[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(f4e(a, e), lds[src + 4 * e * PIX], a2[ct], 0, 0, 0);
                }
            }
        }
        __syncthreads();                 // every wave has finished reading h1
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) H1[(4 * lg + r) * PIX + colb + 16 * ct] = cf_relu(a2[ct][r]);
        if constexpr (DUMP) { rows_store_t<G, HID, HID>(tp.h2, H1, tile, B, wave, lane); plane_mask_store(tp.m2); }
        if constexpr (DBG) dump(H1, HID, C + HID);
        }
    }
    cf_wave_sync();                      // h2: every lane's rows in place before other lanes read them as operands

    // ================= phase 3: [t | raw] = NN.4 h2 + b   (coupling.py:28); reads this wave's own columns of h2 only
    f32x4 acc3[4];
    {
        const float4 b = *reinterpret_cast<const float4*>(ws + G::OFF_SB3 + 4 * lg);
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) { acc3[ct][0] = b.x; acc3[ct][1] = b.y; acc3[ct][2] = b.z; acc3[ct][3] = b.w; }
#pragma unroll
        for (int g = 0; g < G::SG3; ++g) {
            const float4 a = ws_frag(rs, lane, G::OFF_SA3 + g * 256);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (4 * (4 * g + e) < HID) {
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct)
                        acc3[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(f4e(a, e), H1[CF_ROWIDX(4 * (4 * g + e), lg) + colb + 16 * ct],
                                                                        acc3[ct], 0, 0, 0);
                }
        }
    }
    if constexpr (CTX == 1) {            // h = NN(x0) + CN(c): the sample's bias per packed row (coupling.py:39-42)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int ch = chan_of_row16<G>(4 * lg + r);
            const float add = ch >= 0 ? sb[(int64_t)tile * C + ch] : 0.f;
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) acc3[ct][r] += add;
        }
    }
    // ================= affine map and log-det   (coupling.py:52-66)
    if constexpr (LEVEL) cf_wave_sync();      // phase 3 has read h2 (other lanes' rows of these columns): rows <= C are free
    float lsum = 0.f;
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int j = 0; j < 2; ++j)
            if (2 * lg + j < HALF) {
                const float ls = cf_log_scale(acc3[ct][j + 2]);
                if constexpr (LEVEL) {       // [y0 | z1] = the next step's x plane (or the plane the level's epilogue stores)
                    H1[(HALF + 2 * lg + j) * PIX + colb + 16 * ct] = fmaf(acc0[ct][j + 2], __expf(ls), acc3[ct][j]);
                    H1[(2 * lg + j) * PIX + colb + 16 * ct] = Y0[(2 * lg + j) * PIX + colb + 16 * ct];
                } else {
                    Y0[(2 * lg + j) * PIX + colb + 16 * ct] = fmaf(acc0[ct][j + 2], __expf(ls), acc3[ct][j]);     // z1, staged in LDS
                }
                lsum += ls;
                if constexpr (DUMP) {
                    const int64_t o = ((int64_t)tile * HALF + 2 * lg + j) * PIX + colb + 16 * ct;
                    tp.ls[o] = ls;
                    tp.y1[o] = acc0[ct][j + 2];
                }
                if constexpr (DBG) {
                    float* d = dbg + (int64_t)(C + 2 * HID) * dbg_cols + (int64_t)tile * PIX + colb + 16 * ct;
                    d[(int64_t)(2 * lg + j) * dbg_cols] = acc3[ct][j];
                    d[(int64_t)(HALF + 2 * lg + j) * dbg_cols] = acc3[ct][j + 2];
                }
            }
    cf_wave_sync();
    if constexpr (!LEVEL) {
        z_store<G>(z, Y0, tile, HALF, B, wave, lane);
        cf_wave_sync();
    }
    lsum = cf_wave_sum(lsum);
    // the four partial sums: own column of Y0 (its z1 value has been read back by z_store already); LEVEL: of row C of H1 (see above)
    float* const LS = LEVEL ? H1 + C * PIX : Y0;
    if (lane == 0) LS[wave * 64] = lsum;
    __syncthreads();
    if (tid == 0 && tile < B) ldj_acc[tile] += ws[0] + ((LS[0] + LS[64]) + (LS[128] + LS[192]));
}
template <class G, bool SQ, bool DBG = false, bool DUMP = false, int CTX = 0>
__device__ __forceinline__ void flow_step_small_body(const float* x, float* z, float* __restrict__ ldj_acc, const float* __restrict__ ws,
                                                     int B, int64_t xbs, float* __restrict__ dbg, StepTape tp,
                                                     const float* __restrict__ sb = nullptr) {
    constexpr int XI = G::C * G::PTW / 8;
    extern __shared__ __align__(16) float lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float4 xr[XI];
    x_load<G, SQ>(xr, x, xbs, blockIdx.x, B, wave, lane);
    x_to_lds<G, SQ>(xr, lds + G::HALF * G::PIX, wave, lane);
    flow_step_small_phases<G, DBG, DUMP, CTX, false>(z, ldj_acc, ws, B, dbg, tp, sb);
}
template <class G, bool SQ, bool DBG = false, bool DUMP = false, int CTX = 0>
__global__ __launch_bounds__(256, (G::WINO && DUMP) ? 3 : (G::WINO && G::C == 16) ? CF_G16W_MINW : G::MINW) void k_flow_step_small(const float* __restrict__ x, float* __restrict__ z,
                                                                  float* __restrict__ ldj_acc, const float* __restrict__ ws,
                                                                  int B, int64_t xbs, float* __restrict__ dbg, StepTape tp,
                                                                  const float* __restrict__ sb = nullptr) {
    flow_step_small_body<G, SQ, DBG, DUMP, CTX>(x, z, ldj_acc, ws, B, xbs, dbg, tp, sb);
}
// Chained form for small batches (cf_flow_step_fwd_chain): the n <= kChain consecutive flow steps of one resolution level in ONE
// launch.  A workgroup owns whole samples end to end, so step k + 1 can read what step k wrote as soon as the workgroup has passed
// a barrier; steps 2.. run in place on z.  At a batch of 256 a forward is ~20 launches of 10-35 us that a replayed graph issues
// at 7-12 us per node whatever they do: 12 step launches become 3.
template <class G, bool SQ>
__global__ __launch_bounds__(256, (G::WINO && G::C == 16) ? CF_G16W_MINW : G::MINW) void k_flow_step_small_chain(const float* x, float* z, float* __restrict__ ldj_acc,
                                                                                   const WsChain wc, int nsteps, int B, int64_t xbs) {
    flow_step_small_body<G, SQ>(x, z, ldj_acc, wc.ws[0], B, xbs, nullptr, kNoTape);
    for (int st = 1; st < nsteps; ++st) {
        __syncthreads();                 // this workgroup's z of the step before is complete and visible to all of its waves
        flow_step_small_body<G, false>(z, z, ldj_acc, wc.ws[st], B, (int64_t)G::C * G::HW, nullptr, kNoTape);
    }
}
// Level form for saturating batches (cf_flow_step_fwd_level; see k_flow_step_level): z stays in LDS from step to step - one x fetch
// in front of a loop with ONE body, one z store behind it.
template <class G, bool SQ>
__global__ __launch_bounds__(256, (G::WINO && G::C == 16) ? CF_G16W_MINW : G::MINW) void k_flow_step_small_level(const float* __restrict__ x, float* __restrict__ z,
                                                                                   float* __restrict__ ldj_acc, const WsChain wc, int nsteps, int B,
                                                                                   int64_t xbs) {
    constexpr int XI = G::C * G::PTW / 8;
    extern __shared__ __align__(16) float lds[];
    float* H1 = lds + G::HALF * G::PIX;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wave_u = __builtin_amdgcn_readfirstlane(wave);
    {
        float4 xr[XI];
        x_load<G, SQ>(xr, x, xbs, blockIdx.x, B, wave, lane);
        x_to_lds<G, SQ>(xr, H1, wave, lane);
    }
#pragma unroll 1
    for (int st = 0; st < nsteps; ++st) flow_step_small_phases<G, false, false, 0, true>(z, ldj_acc, wc.ws[st], B, nullptr, kNoTape, nullptr, wave_u);
    rows_store<G, G::C>(z, H1, blockIdx.x, 0, B, wave_u, cf_lane_fresh());
}
template <class G>
int launch_step_small_level(const StepArgs& a, const WsChain& wc, int n) {
    const auto k = a.sq ? k_flow_step_small_level<G, true> : k_flow_step_small_level<G, false>;
    k<<<dim3(a.B), dim3(256), (size_t)G::LDS_FLOATS * sizeof(float), a.s>>>(a.x, a.z, a.ldj, wc, n, a.B, a.xbs);
    return 0;
}
// (the launch helpers take the squeeze flag at run time: a.sq picks the SQ instantiation)
template <class G>
int launch_step_small_chain(const StepArgs& a, const WsChain& wc, int n) {
    const auto k = a.sq ? k_flow_step_small_chain<G, true> : k_flow_step_small_chain<G, false>;
    k<<<dim3(a.B), dim3(256), (size_t)G::LDS_FLOATS * sizeof(float), a.s>>>(a.x, a.z, a.ldj, wc, n, a.B, a.xbs);
    return 0;
}

// the specialist coupling (CTX != 0) never sits behind a squeeze: only its SQ = false form is built
template <class G, bool DBG = false, bool DUMP = false, int CTX = 0>
int launch_step_small(const StepArgs& a) {
    auto k = k_flow_step_small<G, false, DBG, DUMP, CTX>;
    if constexpr (CTX == 0) { if (a.sq) k = k_flow_step_small<G, true, DBG, DUMP, CTX>; }
    k<<<dim3(a.B), dim3(256), (size_t)G::LDS_FLOATS * sizeof(float), a.s>>>(a.x, a.z, a.ldj, a.ws, a.B, a.xbs, a.dbg, a.tp, a.sb);
    return 0;
}

}  // namespace
