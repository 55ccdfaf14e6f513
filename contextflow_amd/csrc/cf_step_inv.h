// The inverse flow step: table layout (GeoInv), the two inverse pack kernels, k_flow_step_inv (plain, LD and CTX forms), StepInvArgs
// and the launch helpers.  Included by cf_step.hip (plain and LD forms; beside the headers of the forward families) and
// cf_step_inv_ctx.hip (CTX forms); everything lives in an anonymous namespace of the including translation unit.
#pragma once
#include "cf_step_common.h"
#include <atomic>

namespace {

// ---- inverse step: x = Conv1x1^-1(ActNorm^-1(Coupling^-1(z)))   (coupling.py:68-73, actnorm.py:78, conv1x1.py:72)
// z0 conditions the same three contractions as in the forward direction; y1 = (z1 - t) e^{-log_s}; then
// x = (Wm^-1 diag(e^{logs})) [z0 | y1] + Wm^-1 t  as one more MFMA phase with natural channel rows.
template <class G> struct GeoInv {
    static constexpr int RTI = (G::C + 31) / 32;                 // row tiles of the natural-order output
    static constexpr int OFF_WINV = 0;                           // C*C floats: Wm^-1 (scratch of the prepare step)
    static constexpr int OFF_BI = ((G::C * G::C + 3) / 4) * 4;
    static constexpr int OFF_AI = OFF_BI + RTI * 32;
    static constexpr int WS_FLOATS = OFF_AI + G::NG0 * RTI * 256;
};

template <class G>
__global__ __launch_bounds__(256) void k_step_pack_inv(const float* __restrict__ t, const float* __restrict__ logs,
                                                       float* __restrict__ wsi) {
    using I = GeoInv<G>;
    const int gtid = blockIdx.x * 256 + threadIdx.x, gsz = gridDim.x * 256;
    const float* Winv = wsi + I::OFF_WINV;
    for (int c = gtid; c < I::RTI * 32; c += gsz) {
        float s = 0.f;
        if (c < G::C)
            for (int k = 0; k < G::C; ++k) s = fmaf(Winv[c * G::C + k], t[k], s);
        wsi[I::OFF_BI + c] = s;
    }
    for (int e = gtid; e < G::NG0 * I::RTI * 256; e += gsz) {
        const int j = e & 3, lane = (e >> 2) & 63, q = e >> 8, rt = q % I::RTI, g = q / I::RTI;
        const int row = rt * 32 + (lane & 31), k = 2 * (4 * g + j) + (lane >> 5);
        wsi[I::OFF_AI + e] = (row < G::C && k < G::C) ? Winv[row * G::C + k] * expf(logs[k]) : 0.f;
    }
}

// table of the inverse step's vector-Jacobian product (cf_flow_step_inv_bwd_data): diag(e^{logs}) Wm^-T, the map from the upstream
// d/dx to d/dy, as the A fragments of a dense_phase with the packed rows of phase 0 (OFF_A0 of k_step_pack) - Wm^-1 is the one
// cf_flow_step_inv_prepare left at the head of wsi
template <class G>
__global__ __launch_bounds__(256) void k_step_pack_inv_bwd(const float* __restrict__ wsi, const float* __restrict__ logs,
                                                           float* __restrict__ wsv) {
    const int gtid = blockIdx.x * 256 + threadIdx.x, gsz = gridDim.x * 256;
    const float* Winv = wsi + GeoInv<G>::OFF_WINV;
    for (int e = gtid; e < G::NG0 * G::RT03 * 256; e += gsz) {
        const int j = e & 3, lane = (e >> 2) & 63, q = e >> 8, rt = q % G::RT03, g = q / G::RT03;
        const int ch = chan_of_row<G>(rt * 32 + (lane & 31)), k = 2 * (4 * g + j) + (lane >> 5);
        wsv[e] = (ch >= 0 && k < G::C) ? expf(logs[ch]) * Winv[k * G::C + ch] : 0.f;
    }
}

// LD (cf_flow_step_inv_ld): ld_acc[b] += ws[0] + sum log_s as well - what the forward step adds for its log-det at the recovered
// input x - reduced as flow_step_phases reduces it: lane, shuffles over the lanes of a sample, one LDS hop where a sample spans
// waves, then the one owner of sample b reads, adds and writes (no float atomics: the same bits in every run).  Without the
// flag ld_acc is not read (NULL) and the kernel is the one it was.
// CTX (cf_flow_step_inv_ctx, instantiated in cf_step_inv_ctx.hip): the specialist coupling ALONE backwards - the conditioner takes
// the per-sample bias of conditioner_net's modes 1 / 2, which arrives in the `wsi` argument: no Conv1x1 / ActNorm sits behind that
// coupling, so there is no inverse table, the last dense phase is not run and x = [z0 | (z1 - t) e^{-log_s}] goes from the y plane
// to memory (no un-squeeze: a coupling never sits directly behind a Squeeze).
template <class G, bool LD = false, int CTX = 0>
#ifndef CF_INV16_MINW
#define CF_INV16_MINW 3          // (4 waves per SIMD: 12 spilled registers, 6.55 vs 6.49 ms per cifar10 sample(16384))
#endif
__global__ __launch_bounds__(256, (G::WINO && G::C == 16) ? CF_INV16_MINW : G::MINW) void k_flow_step_inv(const float* __restrict__ z, float* __restrict__ x,
                                                       const float* __restrict__ ws, const float* __restrict__ wsi, int B,
                                                       int64_t zbs, int x_unsq, float* __restrict__ ld_acc) {
    using I = GeoInv<G>;
    static_assert(CTX == 0 || !LD, "the specialist coupling's inverse has no log-det output");
    constexpr int C = G::C, HW = G::HW, PIX = G::PIX, HALF = G::HALF;
    constexpr int PTW = G::PTW, RT03 = G::RT03, NR = (HALF <= 16 ? 8 : 16);
    constexpr int XI = C * PTW / 8;
    extern __shared__ __align__(16) float lds[];
    float* Y0 = lds;
    float* H1 = lds + HALF * PIX;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, lk = lane >> 5;
    const int tile = blockIdx.x, b0 = tile * G::SPW;
    int pix[PTW], pin[PTW];
#pragma unroll
    for (int q = 0; q < PTW; ++q) { pix[q] = (wave * PTW + q) * 32 + li; pin[q] = pix[q] % HW; }

    {   // conditioner input: the first half of z, this wave's columns, straight into the Y0 plane (16-byte accesses)
        float4 zr[XI];
        x_load<G, false>(zr, z, zbs, tile, B, wave, lane);
        x_to_lds<G, false>(zr, H1, wave, lane);                  // z plane: rows [0,HALF) = z0, [HALF,C) = z1
        if constexpr (G::LDS_W > 0) {
            // C = 8: the Winograd-domain weights of the 3x3 into LDS behind the planes (winograd_phase2 reads them there; two
            // workgroup barriers of the conditioner lie between this and their first use)
            const ws_rsrc_t rsw = ws_rsrc(ws, G::WS_FLOATS);
            float* WL = lds + (HALF + G::HID) * PIX;
#pragma unroll
            for (int i = 0; i < G::LDS_W / 1024; ++i)
                *reinterpret_cast<float4*>(WL + (i * 256 + tid) * 4) = ws_frag(rsw, tid, G::OFF_AW + i * 1024);
        }
        cf_wave_sync();
#pragma unroll
        for (int q = 0; q < PTW; ++q)
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const int idx = tile_row(r, lk);
                if (idx < HALF) Y0[idx * PIX + pix[q]] = H1[idx * PIX + pix[q]];
            }
        cf_wave_sync();
    }
    f32x16 acc3[RT03][PTW];
    if constexpr (CTX == 0) {
        conditioner_net<G>(acc3, lds, ws, pix, pin, lane, tid, nullptr, 0, tile);
    } else {
        int soff[PTW];
#pragma unroll
        for (int q = 0; q < PTW; ++q) soff[q] = min(b0 + pix[q] / HW, B - 1) * (CTX == 1 ? C : G::HID);
        conditioner_net<G, CTX>(acc3, lds, ws, pix, pin, lane, tid, nullptr, 0, tile, wsi, soff);
    }
    cf_wave_sync();                      // phase 3 has read h2: its words are reused for the y plane
    // y = [z0 | (z1 - t) e^{-log_s}] as the operand plane of the last phase (this wave's columns of the H region).  z is read a
    // SECOND time here (L2-resident: this workgroup read it a few microseconds ago) instead of being carried in registers
    // across the conditioner: 2 NR PTW registers per lane had cost the Winograd geometries half of their occupancy
    // (140 / 256 / 256 VGPRs at C = 16 / 32 / 64: 2 / 1 / 1 waves per SIMD where the forward kernels run 4 / 2 / 2).
    {
        float4 zr[XI];
        x_load<G, false>(zr, z, zbs, tile, B, wave, lane);
        x_to_lds<G, false>(zr, H1, wave, lane);
        cf_wave_sync();
    }
    [[maybe_unused]] float lsum[PTW];
    if constexpr (LD) {
#pragma unroll
        for (int q = 0; q < PTW; ++q) lsum[q] = 0.f;
    }
#pragma unroll
    for (int q = 0; q < PTW; ++q)
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const int idx = tile_row(r, lk);
            if (idx < HALF) {
                const float tt = acc3[0][q][r];
                const float raw = (HALF <= 16) ? acc3[0][q][r + 8] : acc3[RT03 - 1][q][r];
                const float ls = cf_log_scale(raw);
                float* y1 = &H1[(HALF + idx) * PIX + pix[q]];
                *y1 = (*y1 - tt) * __expf(-ls);
                if constexpr (LD) lsum[q] += ls;
            }
        }
    cf_wave_sync();
    if constexpr (LD) {
        constexpr int SEG = HW < 32 ? HW : 32;            // lanes (pixels) of one sample inside a tile
#pragma unroll
        for (int q = 0; q < PTW; ++q) {
#pragma unroll
            for (int o = 1; o < SEG; o <<= 1) lsum[q] += __shfl_xor(lsum[q], o, 64);
            lsum[q] += __shfl_xor(lsum[q], 32, 64);
        }
        if constexpr (HW <= 32 * PTW) {                   // whole samples inside this wave: the first lane of a sample owns ld_acc[b]
            constexpr int TPS = HW >= 32 ? HW / 32 : 1;   // tiles per sample
#pragma unroll
            for (int q = 0; q < PTW; q += TPS) {
                float sum = lsum[q];
#pragma unroll
                for (int i = 1; i < TPS; ++i) sum += lsum[q + i];
                const int b = b0 + pix[q] / HW;
                if (lk == 0 && (li % SEG) == 0 && b < B) ld_acc[b] += ws[0] + sum;
            }
        } else {
            // a sample spans several waves: one LDS hop through this wave's own columns of Y0 (z0: phase 1 of the conditioner has
            // read it, and nothing reads or writes the plane behind this point)
            constexpr int TPS = HW / 32, WPX = 32 * PTW;
#pragma unroll
            for (int q = 0; q < PTW; ++q)
                if (lane == 0) Y0[wave * WPX + q] = lsum[q];
            __syncthreads();
            if (tid < G::SPW && b0 + tid < B) {
                float sum = 0.f;
#pragma unroll
                for (int i = 0; i < TPS; ++i) {
                    const int t = tid * TPS + i;          // tile index inside the workgroup
                    sum += Y0[(t / PTW) * WPX + (t % PTW)];
                }
                ld_acc[b0 + tid] += ws[0] + sum;
            }
        }
    }
    if constexpr (CTX != 0) {            // the identity front: the y plane (this wave's own columns) is x
        rows_store<G, C>(x, H1, b0, 0, B, wave, lane);
        return;
    }
    f32x16 acc[I::RTI][PTW];
#pragma unroll
    for (int rt = 0; rt < I::RTI; ++rt)
#pragma unroll
        for (int q = 0; q < PTW; ++q) acc[rt][q] = bias_tile(wsi + I::OFF_BI + rt * 32, lk);
    dense_phase<G, G::KS0, G::NG0, I::RTI>(acc, reinterpret_cast<const float4*>(wsi + I::OFF_AI), H1, pix, lane);
    // x tiles -> LDS rows [C, 2C) of the H region (own columns) -> 16-byte stores
    float* Xp = H1 + C * PIX;
#pragma unroll
    for (int rt = 0; rt < I::RTI; ++rt)
#pragma unroll
        for (int q = 0; q < PTW; ++q)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = rt * 32 + tile_row(r, lk);
                if (row < C) Xp[row * PIX + pix[q]] = acc[rt][q][r];
            }
    cf_wave_sync();
    // x_unsq: the step sits behind a Squeeze((2,2)) in the flow - its inverse is an index map of these stores (squeeze.py:13-14)
    if (x_unsq) rows_store_unsq<G>(x, Xp, b0, B, wave, lane);
    else rows_store<G, C>(x, Xp, b0, 0, B, wave, lane);
}

template <class G>
int launch_prepare_inv(const float* Wm, const float* t, const float* logs, float* wsi, hipStream_t s) {
    using I = GeoInv<G>;
    int rc = cf_slogdet_inverse(Wm, G::C, wsi + I::WS_FLOATS, wsi + I::OFF_WINV, (cf_stream_t)s);   // log|det| lands past the tables
    if (rc) return rc;
    k_step_pack_inv<G><<<dim3(16), dim3(256), 0, s>>>(t, logs, wsi);
    return 0;
}

// The operands of one k_flow_step_inv launch by name - the inverse's StepArgs.  ld: the log-det accumulator of the LD form; behind ws a
// form reads the inverse tables wsi (cf_flow_step_inv_prepare; CTX = 0) or the per-sample bias sb (CTX forms: no un-squeeze).
struct StepInvArgs {
    const float* z;
    float *x, *ld = nullptr;
    const float *ws, *wsi = nullptr, *sb = nullptr;
    int B;
    int64_t zbs;
    int x_unsq = 0;
    hipStream_t s;
};

template <class G, bool LD = false, int CTX = 0>
int launch_step_inv(const StepInvArgs& a) {
    constexpr size_t lds_bytes = (size_t)G::LDS_FLOATS * sizeof(float);
    if (lds_bytes > 64 * 1024) {
        static std::atomic<uint64_t> raised{0};
        if (int rc_ = cf_raise_dynamic_lds((const void*)k_flow_step_inv<G, LD, CTX>, 160 * 1024, raised, __func__)) return rc_;
    }
    k_flow_step_inv<G, LD, CTX><<<dim3((a.B + G::SPW - 1) / G::SPW), dim3(256), lds_bytes, a.s>>>(a.z, a.x, a.ws, CTX ? a.sb : a.wsi, a.B,
                                                                                                 a.zbs, a.x_unsq, a.ld);
    return 0;
}

}  // namespace
